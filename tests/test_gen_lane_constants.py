"""The identities behind the generator's lane-constant shortcuts (csrc/vs_dev_generator.h, csrc/vs_dev_primitives.h),
in plain C through gcc with contraction off, as tests/test_div_shortcut.py does:

  a. the jitter recursion's "(double)r / (2147483647 * 10000.0)" as one multiply and two fused multiply-adds
     (vs_jitter_unit_of_draw): the same double as IEEE division for ALL 2^31 draws;
  b. vs_isqrt_floor's short form -- a single-precision square root of the float, one step up, one step down -- against the
     search it replaces (double-precision seed, two loops) for EVERY float in [0, 2^32], with the seed exact and one ulp
     off either way;
  c. K_next == K for Kvar == 0 at draws 0, 1, 2^31 - 2 and 2^31 - 1 (and -0.0 for Kvar), for a set of K;
  d. the falling-flank row a uniform group stages, (Kd*cos[k] - Kd) + 1.0 with Kd = (double)K, padded with 1.0, times the
     cycle's amplitude: the same samples as the expression of the trips, evaluated per cycle with the closing speed the
     cycle's draw gives -- T2 = 4 (the smallest a lane of the short sequences has), 8, 37, 40, 55 (the largest of BASELINE
     config 5) and 100, K = 0.5, 0.65 and 0.8, amplitudes over the admitted range,
     and the pad (cos = 1.0) gives the rising flank 0 and the falling flank ceil(Amplitude).  Given (c) this holds by
     construction for the expression as written HERE: it pins the pad values and the range of amplitudes, not what the
     device stages.  That the kernel evaluates the row in this order, with contraction off, is held by the comparison
     with the oracle on the device alone (tests/test_gpu_gen_lane_constants.py, the uniform cases)."""
import subprocess


def _run(tmp_path, name, src, timeout=1800):
    c = tmp_path / (name + ".c")
    c.write_text(src)
    exe = tmp_path / name
    flags = ["-O2", "-fopenmp", "-ffp-contract=off", "-fno-fast-math"]
    if "fma" in open("/proc/cpuinfo").read():
        flags.append("-mfma")  # hardware fma; without it glibc's exact software fma is used
    subprocess.run(["gcc"] + flags + [str(c), "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, check=True, timeout=timeout)
    return out.stdout.decode().split()


JITTER_DIV = r"""
#include <stdio.h>
#include <math.h>
int main(void) {
  const double C = 2147483647 * 10000.0, inv = 1.0 / C;
  long bad = 0;
  #pragma omp parallel for reduction(+:bad)
  for (long r = 0; r < (1L << 31); r++) {
    double x = (double)r, q0 = x * inv, e = fma(-q0, C, x), q = fma(e, inv, q0);
    if (q != x / C) bad++;
  }
  printf("%ld\n", bad);
  return 0;
}
"""


def test_constant_divisor_of_the_jitter_draw_equals_ieee_division(tmp_path):
    assert _run(tmp_path, "jitterdiv", JITTER_DIV) == ["0"]


ISQRT = r"""
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
static int search(double v) {            /* the function as it was */
  int s = (int)sqrt(v);
  if (s < 0) s = 0;
  while ((double)(s + 1) * (double)(s + 1) <= v) ++s;
  while (s > 0 && (double)s * (double)s > v) --s;
  return s;
}
static int shortform(float seed, double v) {
  int s = (int)seed;
  s += ((double)(s + 1) * (double)(s + 1) <= v) ? 1 : 0;
  s -= ((double)s * (double)s > v) ? 1 : 0;
  return s;
}
int main(void) {
  long bad0 = 0, badu = 0, badd = 0, n = 0;
  #pragma omp parallel for reduction(+:bad0,badu,badd,n)
  for (long b = 0; b <= 0x4F800000L; b++) {   /* the bits of every float from +0 to 2^32 */
    uint32_t u = (uint32_t)b;
    float vf;
    memcpy(&vf, &u, 4);
    const double v = (double)vf;
    const int want = search(v);
    const float seed = sqrtf(vf);
    const float dn = nextafterf(seed, -1.0f);
    if (shortform(seed, v) != want) bad0++;
    if (shortform(nextafterf(seed, INFINITY), v) != want) badu++;
    if (shortform(dn < 0.0f ? 0.0f : dn, v) != want) badd++;
    n++;
  }
  printf("%ld %ld %ld %ld\n", n, bad0, badu, badd);
  return 0;
}
"""


def test_short_integer_square_root_equals_the_search_for_every_float(tmp_path):
    n, exact, up, down = _run(tmp_path, "isqrt", ISQRT)
    assert int(n) == 0x4F800000 + 1
    assert (exact, up, down) == ("0", "0", "0")


KNEXT = r"""
#include <stdio.h>
#include <stdint.h>
static double unit(uint32_t r) { return (double)r / 2147483647.0; }   /* (1.0*random())/RAND_MAX */
int main(void) {
  const uint32_t draws[4] = {0u, 1u, 2147483646u, 2147483647u};
  const float Ks[6] = {0.5f, 0.65f, 0.8f, 1.0f, 3.4e38f, 0.50000006f};
  const float kvars[2] = {0.0f, -0.0f};
  int bad = 0;
  for (int d = 0; d < 4; d++)
    for (int k = 0; k < 6; k++)
      for (int z = 0; z < 2; z++) {
        volatile float K = Ks[k], Kvar = kvars[z];
        const float next = (float)((double)K * (1.0 + (double)(2.0f * Kvar) * (unit(draws[d]) - 0.5)));
        if (next != K) bad++;
      }
  printf("%d\n", bad);
  return 0;
}
"""


def test_closing_speed_is_the_lane_constant_when_kvar_is_zero(tmp_path):
    assert _run(tmp_path, "knext", KNEXT) == ["0"]


FLANK_ROWS = r"""
#include <stdio.h>
#include <stdint.h>
#include <math.h>
#define PI 4.0 * atan(1.0)                 /* flowgen_shimmer.c:39, expands textually */
int main(void) {
  const int T2s[6] = {4, 8, 37, 40, 55, 100};
  const float Ks[3] = {0.5f, 0.65f, 0.8f};
  const uint32_t draws[4] = {0u, 1u, 2147483646u, 2147483647u};
  long bad = 0, n = 0;
  for (int t = 0; t < 6; t++)
    for (int kk = 0; kk < 3; kk++) {
      const int T2 = T2s[t], T2p = (T2 + 7) & ~7;
      double cosrow[104], f[104];
      volatile float K = Ks[kk];
      /* the plan's row (vs_cos_row), the LDS row's pad, and the row a uniform group stages */
      for (int k = 0; k < T2p; k++) cosrow[k] = (k < T2) ? cos(PI * k / T2) : 1.0;
      const double Kd0 = (double)K;
      for (int k = 0; k < T2p; k++) f[k] = (Kd0 * cosrow[k] - Kd0) + 1.0;
      for (int k = T2; k < T2p; k++)
        if (f[k] != 1.0) bad++;
      for (int a = 1; a <= 58980; a += 7) {          /* Amplitude up to (float)1.8 * 32766, in steps that are no divisor of anything here */
        for (int h = 0; h < 2; h++) {
          const float Amplitude = (float)a + (h ? 0.4375f : 0.0f);       /* shimmer leaves fractions */
          const double Ad = (double)Amplitude, Ah = Ad * 0.5;
          /* the cycle's own closing speed, Kvar == 0, any draw */
          volatile float Kvar = 0.0f;
          const double u = (double)draws[(a + h) & 3] / 2147483647.0;
          const double Kd = (double)(float)((double)K * (1.0 + (double)(2.0f * Kvar) * (u - 0.5)));
          for (int k = 0; k < T2p; k++) {
            const int was = (int)ceil(Ad * ((Kd * cosrow[k] - Kd) + 1.0));
            const int now = (int)ceil(Ad * f[k]);
            if (was != now) bad++;
            n++;
          }
          /* the pad of the rising flank is 0 (the uniform group's trips write the 0 themselves), of the falling one ceil(Ad) */
          for (int k = T2; k < T2p; k++) {
            if ((int)ceil(Ah * (1.0 - cosrow[k])) != 0) bad++;
            if ((int)ceil(Ad * f[k]) != (int)ceil(Ad)) bad++;
          }
        }
      }
    }
  printf("%ld %ld\n", n, bad);
  return 0;
}
"""


def test_staged_falling_flank_row_gives_the_samples_of_the_per_cycle_expression(tmp_path):
    n, bad = _run(tmp_path, "flankrows", FLANK_ROWS)
    assert int(n) > 10_000_000 and bad == "0"
