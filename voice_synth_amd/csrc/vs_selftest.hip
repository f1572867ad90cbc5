/*
 * vs_selftest.hip -- the kernels beside the synthesis with their launchers: the device self-test, the wave-to-SIMD probe
 * and the reseeding of a plan's records.
 *
 * Device self-test (vs_ctx_selftest): the shortcuts the synthesis kernels take instead of the reference's
 * library calls are checked against the straightforward form ON THE DEVICE.
 *   [0] vs_unit_of_draw(r) == (double)r / 2147483647.0 (the compiler's IEEE division) for ALL
 *       2^31 possible draws;
 *   [1] Philox4x32-10 known answers (Random123 kat_vectors) and the counter/key wiring;
 *   [2] vs_isqrt_floor(v) == floor(sqrt(v)) for float-valued v on a grid that includes every
 *       perfect square up to 2^24 and its two float neighbours;
 *   [3] vs_round2int(x) against a literal transcription of vowel_new.c:413-427 on a grid around
 *       every half-integer and the clamp edges, tiny negative values and the neighbours of -0.5;
 *   [4] the one-fma noise sample (vs_noise_sample) against the reference's
 *       (short)DC + (short)ceil((r/RAND_MAX)*N - N/2.) for ALL 2^31 draws at 16 (width, DC) pairs,
 *       and for every width 0..VS_NDW_FAST at the edge draws;
 *   [5] vs_philox2 (prepared round keys, two blocks) against vs_philox;
 *   [7] the output-noise sample (vowel -n, vs_out_noise_kernel): (float)(r*inv) against (float)((1.0*r)/RAND_MAX) for ALL
 *       2^31 draws, and y - V_CVT_RPI_I32_F32(-aux), clamped, against round2int(1.0*y + 1.0*aux) for EVERY float aux
 *       (all 2^32 bit patterns but the NaNs and (-2^-38, -0)) at nine y, the packed 16-bit form wherever |aux| <= 32767.
 * bad[k] counts failures of check k ([6] is the host's: the wave-to-SIMD probe).
 */
#include "vs_kernel_table.h"
#include "vs_dev_generator.h"
#include "vs_dev_onoise.h"

__device__ __forceinline__ int vs_round2int_literal(double x)
{
  double dec = x - floor(x);
  if (dec > 0.5) x = x + 1;
  if (x > 32767) x = 32767;
  else if (x < -32767) x = -32767;
  return (int)(int16_t)(int)floor(x);
}
/* both forms of the super-step's rounding against the literal one: vs_round2int() always, the
 * half-down form wherever the super-step would not fall back (vs_superstep); returns the failures */
__device__ __forceinline__ int vs_round2int_check(double x)
{
  const int want = vs_round2int_literal(x);
  int bad = (vs_round2int(x) != want) ? 1 : 0;
  const bool flagged = (__double2hiint(x) <= VS_R2I_Q1_HI) || ((uint32_t)__double2loint(x) == 0xFFFFFFFFu);
  if (!flagged && vs_round2int_half_down(x) != want) bad += 1;
  return bad;
}

/* flowgen_shimmer.c:387, 398, literally */
__device__ __forceinline__ int vs_noise_w_literal(uint32_t r, int N)
{
  return (int)(int16_t)(int)ceil(((1.0 * (double)r) / 2147483647.0) * (double)N - (double)N / 2.);
}

__global__ void __launch_bounds__(256) vs_selftest_kernel(unsigned long long *bad)
{
  const unsigned long long tid = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned long long nthreads = (unsigned long long)gridDim.x * 256ull;
  unsigned long long b0 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b7 = 0;
  for (unsigned long long r = tid; r < (1ull << 31); r += nthreads) {
    const double ref = (1.0 * (double)(uint32_t)r) / 2147483647.0;
    if (vs_unit_of_draw((uint32_t)r) != ref) b0++;
  }
  for (unsigned long long k = tid; k < (1ull << 24); k += nthreads) {
    const float sq = (float)((double)k * (double)k);
    const uint32_t sb = __float_as_uint(sq); /* sq >= 0: neighbours are the adjacent bit patterns */
    const float cand[3] = {sq, __uint_as_float(sb > 0u ? sb - 1u : 0u), __uint_as_float(sb + 1u)};
    for (int j = 0; j < 3; ++j) {
      const double v = (double)cand[j];
      long long want = (long long)k - 2;
      if (want < 0) want = 0;
      while ((double)(want + 1) * (double)(want + 1) <= v) ++want; /* floor(sqrt(v)) by definition */
      if ((long long)vs_isqrt_floor(v) != want) b2++;
    }
  }
  for (unsigned long long k = tid; k < 140000ull * 64ull; k += nthreads) {
    const int base = (int)(k / 64ull) - 70000;             /* integers -70000 .. 69999 */
    const int j = (int)(k % 64ull);
    const double frac = (j < 32) ? 0.5 + (double)(j - 16) * 0x1p-50 : (double)(j - 32) / 32.0;
    const double x = (double)base + frac;
    b3 += vs_round2int_check(x);
    /* the doubles around the integer itself, 16 each way (the largest double below a power of
     * two is where x + 1 rounds up to the next integer) */
    const double xi = __longlong_as_double(__double_as_longlong((double)base) + (long long)(j - 32));
    b3 += vs_round2int_check(xi);
  }
  for (unsigned long long k = tid; k < 4096ull; k += nthreads) {
    /* -2^-e and -0.5 +- j ulps, e = 1..1074: where x - floor(x) rounds */
    const int e = (int)(k % 1075ull);
    const int j = (int)(k / 1075ull);
    const double tiny = -ldexp(1.0, -e) * (1.0 + 0.25 * (double)j);
    const double near = __longlong_as_double(__double_as_longlong(-0.5) + (long long)(e % 9) - 4 + 16 * j);
    b3 += vs_round2int_check(tiny) + vs_round2int_check(near) + vs_round2int_check(-tiny);
    /* the neighbours of +-2^-e: -2^-54 is the last member of the quirk set */
    const double pw = ldexp(1.0, -e);
    for (int d = -2; d <= 2; ++d) {
      const double u = __longlong_as_double(__double_as_longlong(pw) + (long long)d);
      b3 += vs_round2int_check(u) + vs_round2int_check(-u);
    }
  }
  if (tid == 0) {
    /* the quirk set is where the two forms differ, and the super-step's test catches all of it */
    const double q[6] = {-0x1p-54, -0x1p-60, -5e-324, 0x1.fffffffffffffp-1, 0x1.fffffffffffffp+0, 0x1.fffffffffffffp+13};
    for (int i = 0; i < 6; ++i) {
      const bool flagged = (__double2hiint(q[i]) <= VS_R2I_Q1_HI) || ((uint32_t)__double2loint(q[i]) == 0xFFFFFFFFu);
      if (!flagged || vs_round2int(q[i]) != vs_round2int_literal(q[i]) ||
          vs_round2int_half_down(q[i]) + 1 != vs_round2int_literal(q[i]))
        b3++;
    }
  }
  {
    const int widths[16] = {1, 2, 3, 7, 100, 2801, 2802, 4095, 4096, 12345, 32767, 32768, 45001, 65534, 45533, 45534};
    const int dcv[16] = {0, 1, -1, 9830, 0, 0, 3, -3, 0, 0, 16000, -16000, 9830, 0, 9830, -9830};
    for (int wi = 0; wi < 16; ++wi) {
      const int N = widths[wi], dc = dcv[wi];
      const VsNoiseK nk = vs_noise_consts(N, dc);
      for (unsigned long long r = tid; r < (1ull << 31); r += nthreads)
        if ((int)(int16_t)vs_noise_sample(nk, (uint32_t)r) != dc + vs_noise_w_literal((uint32_t)r, N)) b4++;
    }
    const uint32_t edge[12] = {0u, 1u, 2u, 3u, 0x3FFFFFFFu, 0x40000000u, 0x40000001u, 0x7FFFFFFCu, 0x7FFFFFFDu, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x12345678u};
    for (unsigned long long k = tid; k < (unsigned long long)(VS_NDW_FAST + 1) * 12ull; k += nthreads) {
      const int N = (int)(k / 12ull);
      const uint32_t r = edge[k % 12ull];
      const int dc = (N & 1) ? 0 : 7;
      const VsNoiseK nk = vs_noise_consts(N, dc);
      /* widths near the limit leave no room for DC: compare modulo 2^16, as the store does */
      if ((int)(int16_t)vs_noise_sample(nk, r) != (int)(int16_t)(dc + vs_noise_w_literal(r, N))) b4++;
    }
  }
  for (unsigned long long k = tid; k < 65536ull; k += nthreads) {
    const uint32_t blk = (uint32_t)(k * 2654435761ull), k0 = (uint32_t)(k * 40503ull + 1ull), k1 = (uint32_t)(~k * 97ull);
    VsRoundKeys rk;
    vs_round_keys(k0, k1, rk);
    uint32_t o[8], p[8];
    vs_philox2(blk, rk, o);
    vs_philox(blk, k0, k1, p[0], p[1], p[2], p[3]);
    vs_philox(blk + 1u, k0, k1, p[4], p[5], p[6], p[7]);
    for (int w = 0; w < 8; ++w)
      if (o[w] != p[w]) b5++;
  }
  for (unsigned long long r = tid; r < (1ull << 31); r += nthreads) {
    const float want = (float)((1.0 * (double)(uint32_t)r) / 2147483647.0);
    const float got = (float)((double)(uint32_t)r * 0x1.00000002p-31);
    if (got != want) b7++;
  }
  {
    const int ys[9] = {0, 1, -1, 2, 4096, 16384, 32767, -32767, -32768};
    for (unsigned long long k = tid; k < (1ull << 32); k += nthreads) {
      const float aux = __uint_as_float((uint32_t)k);
      if (aux != aux || !vs_onoise_aux_is_plain(aux)) continue;
      const int r = vs_onoise_neg_round(aux);
      const bool narrow = (aux >= -32767.0f) && (aux <= 32767.0f); /* what widths below 65534 give: the packed form */
      for (int j = 0; j < 9; ++j) {
        const int want = vs_round2int_literal(1.0 * (double)ys[j] + 1.0 * (double)aux);
        const long long v = (long long)ys[j] - (long long)r;
        if ((int)((v > 32767) ? 32767 : ((v < -32767) ? -32767 : v)) != want) b7++;
        if (narrow && (int)(int16_t)(vs_onoise_sub2((uint32_t)ys[j] & 0xFFFFu, r, 0) & 0xFFFFu) != want) b7++;
      }
    }
  }
  if (b7) atomicAdd(&bad[7], b7);
  if (b0) atomicAdd(&bad[0], b0);
  if (b2) atomicAdd(&bad[2], b2);
  if (b3) atomicAdd(&bad[3], b3);
  if (b4) atomicAdd(&bad[4], b4);
  if (b5) atomicAdd(&bad[5], b5);
  if (tid == 0) {
    unsigned long long b1 = 0;
    uint32_t o0, o1, o2, o3;
    vs_philox(0u, 0u, 0u, o0, o1, o2, o3);
    if (o0 != 0x6627E8D5u || o1 != 0xE169C58Du || o2 != 0xBC57AC4Cu || o3 != 0x9B00DBD8u) b1++;
    /* counter (n, 0, 0, 0) with a non-trivial key against the host-computed value is covered by
     * every bit-exact parity test; here: the key words are not swapped */
    vs_philox(1u, 2u, 3u, o0, o1, o2, o3);
    uint32_t p0, p1, p2, p3;
    vs_philox(1u, 3u, 2u, p0, p1, p2, p3);
    if (o0 == p0 && o1 == p1) b1++;
    if (b1) atomicAdd(&bad[1], b1);
  }
}

/*
 * Where the hardware puts the wavefronts of a workgroup (vs_ctx_simd_dealing): every wavefront of a workgroup of
 * `blockDim.x / 64` wavefronts that has a CU to itself (the launcher asks for most of the LDS, as the fused launches
 * do) writes its HW_ID register.  The wave-specialised layouts are built on wavefront w running on the SIMD of wavefront w % 4
 * (vs_device.h): correctness does not depend on it, the launch time does (role-major against the wrong order:
 * 2.6 against 6.4 ms, profiles/r04_config4_roles.txt) -- so the plan asks instead of assuming.
 * HW_ID (gfx9 family): wave_id [3:0], simd_id [5:4], pipe_id [7:6], cu_id [11:8], sh_id [12], se_id [15:13].
 */
__global__ void __launch_bounds__(1024) vs_simd_probe_kernel(unsigned *out)
{
  extern __shared__ __attribute__((aligned(16))) int16_t probe_lds[];
  if ((threadIdx.x & (VS_WAVE - 1)) == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4); /* hwreg(HW_REG_HW_ID, 0, 32) */
    out[(size_t)blockIdx.x * 16 + (threadIdx.x >> 6)] = hw | 0x80000000u;     /* bit 31: "written" */
    if (threadIdx.x == 0) probe_lds[0] = (int16_t)hw;                         /* the LDS is really allocated */
  }
  __syncthreads(); /* every wavefront of the workgroup is resident at the same time */
}

/* vs_plan_reseed: record i takes the seeds of the lane it was made from (VsDevLane.row) */
__global__ void __launch_bounds__(256) vs_reseed_kernel(VsDevLane *lanes, const unsigned long long *seeds,
                                                        const unsigned long long *out_seeds, int n_lanes)
{
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n_lanes) return;
  VsDevLane *L = lanes + i;
  const unsigned long long s = seeds[L->row], o = out_seeds[L->row];
  L->key0 = (uint32_t)s;
  L->key1 = (uint32_t)(s >> 32);
  L->okey0 = (uint32_t)o;
  L->okey1 = (uint32_t)(o >> 32);
}

extern "C" hipError_t vs_launch_reseed(VsDevLane *lanes, const unsigned long long *seeds, const unsigned long long *out_seeds,
                                       int n_lanes, hipStream_t stream)
{
  hipLaunchKernelGGL(vs_reseed_kernel, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, stream, lanes, seeds, out_seeds, n_lanes);
  return hipGetLastError();
}

extern "C" hipError_t vs_launch_simd_probe(int waves, unsigned grid, size_t lds_bytes, unsigned *out_dev, hipStream_t stream)
{
  if (waves < 1 || waves > 16) return hipErrorInvalidValue;
  if (lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)vs_simd_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vs_simd_probe_kernel, dim3(grid), dim3((unsigned)waves * VS_WAVE), lds_bytes, stream, out_dev);
  return hipGetLastError();
}

extern "C" hipError_t vs_launch_selftest(unsigned long long *bad_dev, hipStream_t stream)
{
  hipLaunchKernelGGL(vs_selftest_kernel, dim3(4096), dim3(256), 0, stream, bad_dev);
  return hipGetLastError();
}
