/*
 * vs_strack.hip -- gfx950 kernel of the source track (include/voice_synth.h, "source track"): the glottal source of
 * flowgen_shimmer.c:246-423 with a period and an amplitude that follow per-frame arrays already on the device.
 *
 *   vs_strack_kernel: ONE WAVEFRONT PER ROW.  The walk is serial in the row (a cycle's period decides where the next one
 *       begins, and its draws where the next one's start), so what a cycle offers is spread over the lanes:
 *       - the scalar part (frame, period, the jitter and shimmer recursions with their rejection loops, T2, Knew) is
 *         computed by every lane alike from wave-uniform values: the loops are the wavefront's;
 *       - the two flanks 64 samples a trip, lane = sample: the cos row comes from the uploaded table (coalesced, the
 *         host's libm), T4 is the highest and T3 the lowest set bit of a ballot over x < DC;
 *       - the closed phase 64 samples a trip; the noise draws are counter-based, lane k takes the draw of its own
 *         sample from the cycle's first noise draw + its ordinal;
 *       - the cycle is built in LDS (int16) and leaves as contiguous int16 runs of the row;
 *       - x_pow and w_pow are float sums in index order, which no reassociation keeps: the squares are made 64 at a
 *         time, lane = sample, and added one behind the other through scalar registers (st_sum64; w_pow only when the
 *         cycle is logged).
 *       An unvoiced stretch looks for the next voiced frame 64 frames a trip (a ballot) and fills with (short)DC.
 *
 * The general sample-by-sample sequences of the reference only: nothing here relies on a lane's ranges.  Every loop is
 * bounded by the row's length, its frames, a cycle's period or max_reject.  What "cannot happen" (a T2 without a cos
 * row, a cycle beyond the LDS buffer, a stretch that does not advance) sets VS_ST_INTERNAL in the row's status and ends
 * the row's walk.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_device.h"
#include "vs_dev_primitives.h"
#include "vs_strack.h"

/* Philox4x32-10 with the 64-bit block index of the draw contract: counter = (blk_lo, blk_hi, 0, 0) */
__device__ __forceinline__ void st_philox(uint64_t blk, uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
  uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)VS_PHILOX_M0 * c0;
    const uint64_t p1 = (uint64_t)VS_PHILOX_M1 * c2;
    const uint32_t n0 = vs_xor3((uint32_t)(p1 >> 32), c1, k0);
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = vs_xor3((uint32_t)(p0 >> 32), c3, k1);
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += VS_PHILOX_W0;
    k1 += VS_PHILOX_W1;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

/* draw d of the stream: word d & 3 of block d >> 2, shifted right by one */
__device__ __forceinline__ uint32_t st_draw_at(uint64_t d, uint32_t k0, uint32_t k1)
{
  uint32_t o[4];
  st_philox(d >> 2, k0, k1, o);
  const uint32_t lo = (d & 1u) ? o[1] : o[0], hi = (d & 1u) ? o[3] : o[2];
  return ((d & 2u) ? hi : lo) >> 1;
}

/* the row's sequential stream (a block per draw: the scalar draws of a cycle are three and its rejections) */
struct StStream {
  uint64_t d;
  uint32_t k0, k1;
};
__device__ __forceinline__ uint32_t st_draw(StStream &s)
{
  const uint32_t v = st_draw_at(s.d, s.k0, s.k1);
  s.d += 1u;
  return v;
}

__device__ __forceinline__ float st_sq(int x)
{
  const float f = (float)x;
  return f * f;
}

/* acc + v[0] + v[1] + ... + v[63], one float addition behind the other in lane order: the reference's power sums
 * (fg:375, 388) cannot be reassociated.  The squares are made lane-parallel (each rounds on its own); only the additions
 * are serial, on values read lane by lane into scalar registers -- no LDS round trip per sample.  A lane outside the sum
 * brings +0.0f, which changes no partial sum (they are never negative zero). */
__device__ __forceinline__ float st_sum64(float acc, float v)
{
  const int bits = __builtin_bit_cast(int, v);
#pragma unroll
  for (int k = 0; k < 64; ++k) acc += __builtin_bit_cast(float, __builtin_amdgcn_readlane(bits, k));
  return acc;
}

/* (int)sqrt(v) of fg:382 for the arguments a valid lane can reach: x_pow <= 32767^2, the factor in front of it below
 * 24 and noise >= 1 (vs_lane_validate), so v < 2^35, or v is NaN or -0 (both give 0).  The device's root only seeds
 * the answer; two exact steps either way settle it (the products are exact below 2^53).  Without loops: the search
 * loops of vs_isqrt_floor, unrolled on wave-uniform values, are what made this kernel run out of scalar registers. */
__device__ __forceinline__ int st_isqrt_floor(double v)
{
  int s = (int)__builtin_sqrt(v);
  s = s < 0 ? 0 : s;
#pragma unroll
  for (int k = 0; k < 2; ++k) s += ((double)(s + 1) * (double)(s + 1) <= v) ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) s -= (s > 0 && (double)s * (double)s > v) ? 1 : 0;
  return s;
}

__global__ __launch_bounds__(64) void vs_strack_kernel(VsStArgs a)
{
  __shared__ int16_t xbuf[VS_ST_CYCLE_MAX]; /* the cycle */
  __shared__ int16_t wbuf[VS_ST_CYCLE_MAX]; /* its noise values in draw order (logged cycles only) */
  const long row = blockIdx.x;
  const int lane = threadIdx.x;
  const VsStRow R = a.rows[row];
  const char *per = a.period + row * a.frames_pitch * a.period_stride;
  const char *ampt = a.amp ? a.amp + row * a.frames_pitch * a.amp_stride : nullptr;
  int16_t *out = a.out + row * a.out_pitch;
  vs_strack_cycle *logrow = a.cycles ? a.cycles + row * a.cycles_pitch : nullptr;
  const int32_t *toff = a.toff;
  const double *costab = a.costab;
  vs_strack_stat *stat = a.stat + row;
  /* (addresses of per-lane loads and stores: kept in vector registers, the scalar ones are all taken) */
  asm volatile("" : "+v"(out), "+v"(logrow), "+v"(toff), "+v"(costab), "+v"(stat));
  const int F = R.n_frames, len = R.length;

  /* frame f: its period and amplitude, and whether it is voiced */
  auto frame = [&](int f, int &P, int &A0) -> bool {
    P = *(const int32_t *)(per + (long)f * a.period_stride);
    A0 = ampt ? *(const int32_t *)(ampt + (long)f * a.amp_stride) : R.amp;
    return P >= R.pmin && P <= R.pmax && (!ampt || (A0 >= 0 && A0 <= 32766));
  };

  StStream rng;
  rng.d = 0;
  rng.k0 = R.key0;
  rng.k1 = R.key1;
  /* the stream lives in vector registers (every lane the same values): as wave-uniform values the compiler keeps the
   * Philox rounds and the cached block in scalar registers and runs out of them */
  asm volatile("" : "+v"(rng.k0), "+v"(rng.k1));
  float dp0 = 0.0f, ds0 = 0.0f;
  int T4 = 0, g = 0;
  bool prev = false;
  int Pp = 0, Ap = 0;
  int status = 0, n_cycles = 0, n_resets = 0, n_unvoiced = 0;
  asm volatile("" : "+v"(status), "+v"(n_cycles), "+v"(n_resets), "+v"(n_unvoiced)); /* (counted, never steered by) */

  while (g < len) {
    /* (0 <= g - offset < 2^32 for g >= offset: the 64-bit quotient of the definition from a 32-bit division) */
    const int f = g < R.offset ? 0 : (int)min(((unsigned)g - (unsigned)R.offset) / (unsigned)R.hop, (unsigned)(F - 1));
    int P, A0;
    if (!frame(f, P, A0)) {
      /* ---- unvoiced: up to the first sample of the next voiced frame ---- */
      int f2 = F;
      for (int base = f + 1; base < F; base += 64) {
        const int ff = base + lane;
        int p2 = 0, a2 = 0;
        const bool v = ff < F && frame(ff, p2, a2);
        const unsigned long long m = __ballot(v);
        if (m) {
          f2 = base + __builtin_ctzll(m);
          break;
        }
      }
      const long long e64 = f2 < F ? min((long long)R.offset + (long long)f2 * (long long)R.hop, (long long)len) : (long long)len;
      const int e = (int)e64;
      if (e <= g) { /* cannot happen: f2 > f(g) */
        status |= VS_ST_INTERNAL;
        break;
      }
      for (int i = g + lane; i < e; i += 64) out[i] = (int16_t)R.dcs;
      n_unvoiced += e - g;
      g = e;
      dp0 = 0.0f;
      ds0 = 0.0f;
      T4 = 0;
      prev = false;
      continue;
    }

    /* ---- a cycle ---- */
    if (prev) {
      if (P != Pp) {
        dp0 = (float)((double)dp0 * (double)P / (double)Pp);
        T4 = 0;
      }
      if (A0 != Ap) ds0 = Ap ? (float)((double)ds0 * (double)A0 / (double)Ap) : 0.0f;
    }
    /* jitter: fg:248-291 */
    int T = P;
    if (R.flags & VS_STF_JITTER) {
      const float dp1 = dp0, t_hi = (float)1.2 * (float)P, t_lo = (float)0.8 * (float)P;
      for (int rej = 0;;) {
        const uint32_t r = st_draw(rng);
        const float J = (float)(vs_jitter_unit_of_draw(r) * 40000.0 * (double)R.jitter - 2.0 * (double)R.jitter);
        const double Jd = (double)J;
        dp0 = (float)((double)dp1 * (2.0 + Jd) / (2.0 - Jd) + 2.0 * (double)P * Jd / (2.0 - Jd));
        T = vs_short_of(ceil((double)((float)P + dp0)));
        if (!(((float)T > t_hi) || ((float)T < t_lo))) break;
        if (++rej >= a.max_reject) {
          T = P;
          dp0 = 0.0f;
          n_resets++;
          break;
        }
      }
    }
    /* shimmer: fg:293-313 */
    float Amplitude = (float)A0, S = 0.0f;
    if (R.flags & VS_STF_SHIMMER) {
      const float ds1 = ds0, a_hi = (float)1.8 * (float)A0, a_lo = (float)0.2 * (float)A0;
      for (int rej = 0;;) {
        const uint32_t r = st_draw(rng);
        const float epsilon = (float)r / 2147483648.0f; /* (float)RAND_MAX == 2^31 */
        S = (float)((double)epsilon * 4.0 * (double)R.shimmer - 2.0 * (double)R.shimmer);
        const double Sd = (double)S;
        ds0 = (float)((double)ds1 * (2.0 + Sd) / (2.0 - Sd) + 2.0 * (double)A0 * Sd / (2.0 - Sd));
        Amplitude = (float)A0 + ds0;
        if (!((Amplitude > a_hi) || (Amplitude < a_lo))) break;
        if (++rej >= a.max_reject) {
          Amplitude = (float)A0;
          ds0 = 0.0f;
          n_resets++;
          break;
        }
      }
    }
    T = __builtin_amdgcn_readfirstlane(T);
    const int T2 = __builtin_amdgcn_readfirstlane((int)ceil(0.5 * (double)R.cq * (double)P));
    const int tab = __builtin_amdgcn_readfirstlane((T2 >= 1 && T2 <= VS_ST_T2_MAX) ? toff[T2] : -1);
    if (tab < 0 || T2 < 1 || 2 * T2 > VS_ST_CYCLE_MAX || T < 1 || T > VS_ST_CYCLE_MAX) { /* cannot happen */
      status |= VS_ST_INTERNAL;
      break;
    }
    const double *crow = costab + tab;
    const double Ad = (double)Amplitude, Ah = Ad * 0.5; /* "Amplitude * 0.5 * (...)" evaluates (Amplitude*0.5) first */

    __syncthreads(); /* the cycle before has left xbuf */
    /* rising half-pulse: fg:318-324 */
    for (int base = 0; base < T2; base += 64) {
      const int i = base + lane;
      bool lt = false;
      if (i < T2) {
        int x = vs_short_of(ceil(Ah * (1.0 - crow[i])));
        lt = (float)x < R.DC; /* if(x[i] < par.DC) { x[i] = par.DC; T4 = i; } */
        x = lt ? R.dcs : x;
        xbuf[i] = (int16_t)x;
      }
      const unsigned long long m = __ballot(lt);
      if (m) T4 = base + 63 - __builtin_clzll(m);
    }
    /* closing speed: fg:325 */
    const uint32_t rk = st_draw(rng);
    const double Kd = (double)(float)((double)R.K * (1.0 + (double)(2.0f * R.Kvar) * (vs_unit_of_draw(rk) - 0.5)));
    /* falling half-pulse: fg:327-332 */
    int T3 = 2 * T2;
    for (int k0 = 0; k0 < T2; k0 += 64) {
      const int k = k0 + lane;
      bool brk = false;
      if (k < T2) {
        const int x = vs_short_of(ceil(Ad * ((Kd * crow[k] - Kd) + 1.0)));
        brk = (float)x < R.DC; /* if(x[i] < par.DC) break; */
        xbuf[T2 + k] = (int16_t)x; /* (at and behind the break: written again below, or beyond T) */
      }
      const unsigned long long m = __ballot(brk);
      if (m) {
        T3 = T2 + k0 + __builtin_ctzll(m);
        break;
      }
    }
    __syncthreads();
    /* closed phase: fg:334-336 */
    for (int i = T3 + lane; i < T; i += 64) xbuf[i] = (int16_t)R.dcs;

    const bool logged = logrow && n_cycles < a.cycles_pitch;
    float x_pow = 0.0f, w_pow = 0.0f;
    if (R.flags & VS_STF_NOISE) {
      /* closed-phase noise: fg:373-411 */
      __syncthreads();
      float psum = 0.0f;
      for (int c0 = T4 & ~63; c0 < T3; c0 += 64) {
        const int i = c0 + lane;
        psum = st_sum64(psum, (i >= T4 && i < T3) ? st_sq((int)xbuf[i]) : 0.0f);
      }
      x_pow = psum / ((float)T3 - (float)T4);
      const float aux = (float)(1.0 + (double)(((float)T3 - (float)T4) / ((float)T)));
      const float arg = 12.0f * aux * x_pow / R.noise;
      const int NDW = __builtin_amdgcn_readfirstlane(st_isqrt_floor((double)arg));
      const double NDWd = (double)NDW, half = NDWd / 2.0;
      const int m = T4 + (T > T3 ? T - T3 : 0); /* draws of this cycle: [0, T4) then [T3, T) */
      const uint64_t d0 = rng.d;
      for (int q0 = 0; q0 < m; q0 += 64) {
        const int q = q0 + lane;
        if (q < m) {
          const uint32_t r = st_draw_at(d0 + (uint64_t)q, rng.k0, rng.k1);
          /* w[i] = (short)ceil(((1.0*random())/RAND_MAX)*NDW - NDW/2.0); x[i] = truncate((float)x[i] + w[i]) */
          const int wv = vs_short_of(ceil(vs_unit_of_draw(r) * NDWd - half));
          const int i = q < T4 ? q : T3 + (q - T4);
          int xv = (q < T4 ? (int)xbuf[i] : R.dcs) + wv;
          xv = (xv > 32767) ? 32767 : ((xv < -32767) ? -32767 : xv);
          xbuf[i] = (int16_t)xv;
          if (logged) wbuf[q] = (int16_t)wv;
        }
      }
      rng.d = d0 + (uint64_t)m;
      if (logged) {
        __syncthreads();
        float wsum = 0.0f;
        for (int q0 = 0; q0 < m; q0 += 64) wsum = st_sum64(wsum, q0 + lane < m ? st_sq((int)wbuf[q0 + lane]) : 0.0f);
        w_pow = wsum / (float)T;
      }
    }
    if (logged && lane == 0) {
      vs_strack_cycle rec;
      rec.start = g;
      rec.T = T;
      rec.frame = f;
      rec.amp = A0;
      rec.S = S;
      rec.x_pow = x_pow;
      rec.w_pow = w_pow;
      rec.reserved_ = 0;
      logrow[n_cycles] = rec;
    }
    /* emit: fg:413-421 */
    __syncthreads();
    const int lim = min(T, len - g);
    for (int i = lane; i < lim; i += 64) out[g + i] = xbuf[i];
    n_cycles++;
    g = (int)min((long long)g + (long long)T, (long long)len);
    prev = true;
    Pp = P;
    Ap = A0;
  }
  if (lane == 0) {
    vs_strack_stat st;
    st.status = status | (n_cycles == 0 ? VS_ST_NO_VOICED : 0);
    st.n_cycles = n_cycles;
    st.n_resets = n_resets;
    st.n_unvoiced = n_unvoiced;
    st.n_draws = rng.d;
    *stat = st;
  }
}

extern "C" hipError_t vs_launch_strack(const VsStArgs *args, hipStream_t stream)
{
  if (args->n_lanes <= 0 || args->n_lanes > 0x7FFFFFFFL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(vs_strack_kernel, dim3((unsigned)args->n_lanes), dim3(64), 0, stream, *args);
  return hipGetLastError();
}
