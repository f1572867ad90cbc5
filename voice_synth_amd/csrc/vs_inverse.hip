/*
 * vs_inverse.hip -- gfx950 kernels of the inverse filter (include/voice_synth.h, "inverse filtering"): A(z) as an FIR
 * filter on int16 speech rows in HBM behind the de-emphasis u[n] = s[n] + rho*u[n-1], with the coefficient set that
 * vs_track would run at the same sample of the same row.
 *
 * One row per lane, 64-lane workgroups (one wavefront), templated on the arithmetic, the window class and the mode.  The
 * lanes per workgroup, the window classes and the LDS plan are the coefficient tracks' (vs_track.h), and so are the set
 * walk, the usability tests and the step-down / step-up below: they restate vs_track.hip operation for operation, without
 * the per-set gains, so that the same row selects the same taps at the same sample in both.
 *
 *   - The rotating register window with static indices (24 doubles for orders up to 22, 48 for 23..40; the wide class
 *     alternates between the two halves, a scalar branch) holds u, the de-emphasised INPUT, not the output: the output of
 *     a sample feeds nothing.
 *   - The taps live in VGPRs (P of them: the class's maximum).  Lower orders carry zeros in the missing taps:
 *     e + 0*u == e for finite u (up to the sign of a zero, which cannot reach the int16 output), and u is always finite
 *     (|u[n]| <= 32768*(n + 1) for 0 <= rho <= 1).
 *   - The samples of a pass do not depend on one another; only u does, through one multiply and one add per sample.  So
 *     there is no scheduling barrier between the samples (the compiler interleaves their tap sums), and the 16-byte
 *     loads of the NEXT pass are issued before the arithmetic of the current one: at 65536 rows there is one wavefront
 *     per SIMD, and nothing else hides the latency of HBM.
 *   - 16-byte loads and stores on whole groups of eight samples when every row start is 4-byte aligned; the scalar path
 *     otherwise and on the tail.
 *   - Which set, the one test per set in order, the sets behind the last sample (for n_unusable), hold and glide, ka / kb
 *     in LDS [2][P][64]: as vs_track.hip has them.
 *
 * Per-row status and the count of clipped samples go into vs_inverse_stat; there is no device trap.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_inverse.h"

typedef uint32_t inv_u32x4 __attribute__((ext_vector_type(4), aligned(4))); /* 16 bytes of a PCM row: rows are only 4-byte aligned */

#define INV_GROUPS (VS_TRACK_GROUP / 8) /* groups of eight samples per pass */

/* round2int() of vowel_new.c:413-427 as the track kernels have it (vs_dev_primitives.h has the reasoning), before its
 * clamp: the floor, held to [-32768, 32768] as a double, so that the conversion is in range whatever the size of x (past
 * int32 too; a NaN, where nothing is promised, comes out as -32768).  The clamp changes the value where the result lies
 * outside [-32767, 32767]: inv_clamped(). */
__device__ __forceinline__ int inv_round(double x)
{
  const double dec = __builtin_amdgcn_fract(x);
  x = x + ((dec > 0.5) ? 1.0 : 0.0);
  return (int)fmin(fmax(floor(x), -32768.0), 32768.0);
}
__device__ __forceinline__ unsigned inv_clamped(int v) { return ((unsigned)(v + 32767) > 65534u) ? 1u : 0u; }
__device__ __forceinline__ int inv_clamp(int v) { return (v > 32767) ? 32767 : ((v < -32767) ? -32767 : v); }

__device__ __forceinline__ bool inv_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

/* hold: A[1..p] finite */
__device__ __forceinline__ bool inv_set_finite(const double *__restrict__ c, int p)
{
  bool ok = true;
  for (int j = 1; j <= p; ++j) ok = ok && inv_finite(c[j]);
  return ok;
}

template <int P>
__device__ __forceinline__ void inv_load_taps(double (&a)[P + 1], const double *__restrict__ c, int p)
{
#pragma unroll
  for (int j = 1; j <= P; ++j) a[j] = (j <= p) ? c[j] : 0.0;
}

/* glide: the set's usability test and its step-down into the lane's LDS slot S (S[(i - 1) * 64] = k_i); the slot's
 * content is undefined after a failure */
__device__ __forceinline__ bool inv_step_down(double *S, const double *__restrict__ c, int p)
{
  bool ok = true;
  for (int j = 1; j <= p; ++j) {
    const double v = c[j];
    ok = ok && inv_finite(v);
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

/* the 16-byte loads of the pass that starts at sample m: the whole groups only (the others are read sample by sample,
 * under their bounds, when their pass runs) */
__device__ __forceinline__ void inv_fetch(inv_u32x4 (&v)[INV_GROUPS], const int16_t *__restrict__ irow, int m, int len, bool vec)
{
#pragma unroll
  for (int g = 0; g < INV_GROUPS; ++g) {
    const int n0 = m + 8 * g;
    const inv_u32x4 zero = {0u, 0u, 0u, 0u};
    v[g] = zero;
    if (vec && n0 >= 0 && n0 + 8 <= len) v[g] = *(const inv_u32x4 *)(irow + n0);
  }
}

/* one pass of VS_TRACK_GROUP samples from sample m on window positions T0 .. T0 + 23; in: what inv_fetch loaded for it */
template <int ARITH, int P, int SS, int T0>
__device__ __forceinline__ void inv_pass(const double (&a)[P + 1], double (&u)[SS], const inv_u32x4 (&in)[INV_GROUPS],
                                         const int16_t *__restrict__ irow, int16_t *__restrict__ orow, int m, int len,
                                         bool vec, double rho, double scale, int *clipped)
{
#pragma unroll
  for (int g = 0; g < INV_GROUPS; ++g) {
    const int n0 = m + 8 * g;
    const bool whole = vec && (n0 + 8 <= len);
    int xin[8];
    if (whole) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xin[2 * e] = (int)(int16_t)(in[g][e] & 0xFFFFu);
        xin[2 * e + 1] = (int)(int16_t)(in[g][e] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) xin[k] = (n0 + k < len) ? (int)irow[n0 + k] : 0;
    }
    int outv[8];
    unsigned cbits = 0; /* bit k: sample n0 + k went through the clamp */
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int t = T0 + 8 * g + k;
      const double u1 = u[(t + SS - 1) % SS];
      /* the de-emphasis: the one chain that runs from sample to sample */
      const double un = (ARITH == VS_ARITH_EXACT) ? ((double)xin[k] + rho * u1) : __builtin_fma(rho, u1, (double)xin[k]);
      u[t] = un; /* the window rotates by renaming */
      double e;
      if (ARITH == VS_ARITH_EXACT) {
        e = un;
#pragma unroll
        for (int j = 1; j <= P; ++j) e = e + a[j] * u[(t + SS - j) % SS];
      } else {
        double p0 = un, p1 = a[2] * u[(t + SS - 2) % SS];
#pragma unroll
        for (int j = 3; j <= P; ++j) {
          const double uj = u[(t + SS - j) % SS];
          if (j & 1) p0 = __builtin_fma(a[j], uj, p0);
          else p1 = __builtin_fma(a[j], uj, p1);
        }
        e = __builtin_fma(a[1], u1, p0 + p1);
      }
      const int v = inv_round(e * scale);
      cbits |= inv_clamped(v) << k;
      outv[k] = inv_clamp(v);
    }
    if (whole) {
      inv_u32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ((uint32_t)outv[2 * e] & 0xFFFFu) | ((uint32_t)outv[2 * e + 1] << 16);
      *(inv_u32x4 *)(orow + n0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (n0 + k < len) orow[n0 + k] = (int16_t)outv[k];
    }
    /* n_clipped counts the samples inside the row */
    const int inside = len - n0;
    *clipped += __popc(cbits & ((inside >= 8) ? 0xFFu : ((inside <= 0) ? 0u : ((1u << inside) - 1u))));
  }
}

template <int ARITH, int P, int MODE>
__global__ void __launch_bounds__(VS_TRACK_LANES) vs_inverse_kernel(VsInverseArgs args)
{
  constexpr int SS = (P <= VS_TRACK_P0) ? VS_TRACK_GROUP : 2 * VS_TRACK_GROUP;
  extern __shared__ double inv_lds[]; /* glide: [2][P][64] */
  const int lane = (int)threadIdx.x;
  const long gl = (long)blockIdx.x * VS_TRACK_LANES + lane;
  if (gl >= args.n_lanes) return; /* (no barrier below) */
  const vs_inverse_row R = args.rows[gl];
  const int p = args.order, K = R.n_sets;
  int len = R.length;
  const long long hop = R.hop;
  const double rho = (double)R.de_emphasis, scale = (double)R.scale;
  const double *__restrict__ cs = args.coefs + gl * args.sets_pitch * (long)(p + 1);
  const int16_t *__restrict__ irow = args.in + gl * args.in_pitch;
  int16_t *__restrict__ orow = args.out + gl * args.out_pitch;
  const bool vec = args.vec_ok != 0;
  const long cstride = p + 1;

  double a[P + 1];
  double u[SS];
#pragma unroll
  for (int j = 0; j <= P; ++j) a[j] = 0.0;
#pragma unroll
  for (int j = 0; j < SS; ++j) u[j] = 0.0; /* u[n] = 0 for n < 0 */
  int sa = 0; /* glide: the slot of ka; kb is in the other */
  double *const S0 = inv_lds + lane;
#define INV_SLOT(s) (S0 + (long)(s) * (P * VS_TRACK_LANES))

  /* E_{-1}: the first usable set */
  int nt = 0, nun = 0; /* sets tested so far, unusable ones among them */
  bool have = false;
  while (nt < K && !have) {
    const double *c = cs + nt * cstride;
    if (MODE == VS_TRACK_HOLD) {
      have = inv_set_finite(c, p);
      if (have) inv_load_taps<P>(a, c, p);
    } else {
      have = inv_step_down(INV_SLOT(0), c, p);
    }
    if (!have) nun++;
    nt++;
  }
  if (!have) { /* VS_INVERSE_NO_SET: zeros */
    for (int n = 0; n < len; ++n) orow[n] = 0;
    len = 0;
  }

  int kc = 0;                                  /* the k of the pass */
  long long nextb = (long long)R.offset + hop; /* the sample at which k = kc + 1 begins */
  /* glide: kb = the reflection coefficients of E_{kc+1} into the free slot; set kc + 1 is tested here if it has not been
   * (those up to the first usable set have: E_{kc+1} is E_kc then, as it is behind the last set) */
#define INV_FILL_KB()                                            \
  {                                                              \
    const int cand = kc + 1;                                     \
    bool ok = false;                                             \
    if (cand < K && cand >= nt) {                                \
      nt = cand + 1;                                             \
      ok = inv_step_down(INV_SLOT(sa ^ 1), cs + cand * cstride, p); \
      if (!ok) nun++;                                            \
    }                                                            \
    if (!ok) {                                                   \
      const double *src = INV_SLOT(sa);                          \
      double *dst = INV_SLOT(sa ^ 1);                            \
      for (int i = 0; i < p; ++i) dst[i * VS_TRACK_LANES] = src[i * VS_TRACK_LANES]; \
    }                                                            \
  }
  if (MODE == VS_TRACK_GLIDE && have) INV_FILL_KB();

  int last_k = -1;
  double last_t = 0.0;
  int half = 0;
  int clipped = 0;
  inv_u32x4 nxt[INV_GROUPS];
  inv_fetch(nxt, irow, 0, len, vec);
  for (int m = 0; m < len; m += VS_TRACK_GROUP) {
    inv_u32x4 cur[INV_GROUPS];
#pragma unroll
    for (int g = 0; g < INV_GROUPS; ++g) cur[g] = nxt[g];
    /* the next pass's loads, ahead of this pass's set walk and arithmetic (m + 24 cannot wrap: a pass that follows has
     * m + 24 < len) */
    if (m < len - VS_TRACK_GROUP) inv_fetch(nxt, irow, m + VS_TRACK_GROUP, len, vec);
    while (kc < K - 1 && (long long)m >= nextb) { /* skipped by the wavefront when no lane's k moves */
      kc++;
      nextb += hop;
      if (MODE == VS_TRACK_HOLD) {
        if (kc >= nt) {
          const double *c = cs + kc * cstride;
          nt = kc + 1;
          if (inv_set_finite(c, p)) inv_load_taps<P>(a, c, p);
          else nun++;
        }
      } else {
        sa ^= 1;
        INV_FILL_KB();
      }
    }
    if (MODE == VS_TRACK_GLIDE) {
      double t = 0.0;
      if ((long long)m >= (long long)R.offset && kc < K - 1) t = (double)((long long)m - (nextb - hop)) / (double)hop;
      if (kc != last_k || t != last_t) {
        last_k = kc;
        last_t = t;
        const double *Ka = INV_SLOT(sa), *Kb = INV_SLOT(sa ^ 1);
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
      }
    }
    if (SS == VS_TRACK_GROUP || half == 0) inv_pass<ARITH, P, SS, 0>(a, u, cur, irow, orow, m, len, vec, rho, scale, &clipped);
    else inv_pass<ARITH, P, SS, SS - VS_TRACK_GROUP>(a, u, cur, irow, orow, m, len, vec, rho, scale, &clipped);
    half ^= 1;
  }

  /* the sets the row did not reach: tested for n_unusable only (glide: in kb's slot, which nothing reads any more) */
  for (; nt < K; ++nt) {
    const double *c = cs + nt * cstride;
    const bool ok = (MODE == VS_TRACK_HOLD) ? inv_set_finite(c, p) : inv_step_down(INV_SLOT(sa ^ 1), c, p);
    if (!ok) nun++;
  }
  if (args.stat) {
    vs_inverse_stat st;
    st.status = have ? 0 : VS_INVERSE_NO_SET;
    st.n_unusable = nun;
    st.n_clipped = clipped;
    st.reserved_ = 0;
    args.stat[gl] = st;
  }
#undef INV_FILL_KB
#undef INV_SLOT
}

template <int ARITH, int P>
static hipError_t inv_launch(int mode, const VsInverseArgs *args, unsigned grid, hipStream_t stream)
{
  if (mode == VS_TRACK_HOLD) {
    hipLaunchKernelGGL((vs_inverse_kernel<ARITH, P, VS_TRACK_HOLD>), dim3(grid), dim3(VS_TRACK_LANES), 0, stream, *args);
  } else {
    const size_t lds = (size_t)vs_track_lds_doubles(P) * sizeof(double);
    hipLaunchKernelGGL((vs_inverse_kernel<ARITH, P, VS_TRACK_GLIDE>), dim3(grid), dim3(VS_TRACK_LANES), lds, stream, *args);
  }
  return hipGetLastError();
}

extern "C" hipError_t vs_launch_inverse(int arith, int mode, const VsInverseArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0) return hipSuccess;
  if (args->order < 1 || args->order > VS_MAX_ORDER || (mode != VS_TRACK_HOLD && mode != VS_TRACK_GLIDE))
    return hipErrorInvalidValue;
  const long blocks = (args->n_lanes + VS_TRACK_LANES - 1) / VS_TRACK_LANES;
  if (blocks > 0x7FFFFFFFL) return hipErrorInvalidValue;
  const bool wide = args->order > VS_TRACK_P0;
  /* (VS_ARITH_F32 as well: like the track kernels, the inverse has no single-precision form) */
  if (arith == VS_ARITH_EXACT)
    return wide ? inv_launch<VS_ARITH_EXACT, VS_TRACK_P1>(mode, args, (unsigned)blocks, stream)
                : inv_launch<VS_ARITH_EXACT, VS_TRACK_P0>(mode, args, (unsigned)blocks, stream);
  return wide ? inv_launch<VS_ARITH_FMA, VS_TRACK_P1>(mode, args, (unsigned)blocks, stream)
              : inv_launch<VS_ARITH_FMA, VS_TRACK_P0>(mode, args, (unsigned)blocks, stream);
}
