/* One of the five analysis programs (acoustic, formants, glottal, vtrack, vinverse) as it is -- its source included here
 * with main renamed, -DCLI_SOURCE='"../../voice_synth_amd/cli/acoustic.c"' -- on a stand-in device: the library's real
 * host side (vs_api.c, vs_blocks.c, vs_planhost.c, vs_host.c and the six vs_*_host.c) against the stand-in HIP runtime of
 * hip_standin.h and the stand-in launchers below.  A launcher computes nothing a kernel computes: per row it hashes
 * everything it was given -- the call's scalars, the row's record, the row's samples, the sets -- and spreads that hash
 * over every field of every record and every sample it writes, so that a wrong pitch, length, padding, option or pointer
 * changes what the program prints or writes.  Some hash values give NaN fields, status bits, no marks, so that those
 * branches of the printers are reached.  Arrays that must stay NULL are CHECKed.
 * VS_STANDIN_FAIL_AT=n (read here only) makes the n-th runtime call of the process fail.
 * tests/test_cli_trace.py builds one executable per program under ASan/UBSan, runs the cases of its table with leak
 * detection and compares status, stdout, stderr and the output files with tests/golden/cli_trace.txt.  Host logic only:
 * what the kernels make of the same arguments is the GPU tests' of each program. */
#define STANDIN_COPY_DOWN 1
#define STANDIN_FILL 0xA5
#define STANDIN_NULL_STREAM 1 /* the programs never set a stream */
#define STANDIN_DEVICES 2     /* VS_DEVICE=1 */
#include <math.h>

#include "../../voice_synth_amd/csrc/vs_internal.h"
#include "../../voice_synth_amd/csrc/vs_acoustic.h"
#include "../../voice_synth_amd/csrc/vs_glottal.h"
#include "../../voice_synth_amd/csrc/vs_iaif.h"
#include "../../voice_synth_amd/csrc/vs_inverse.h"
#include "hip_standin.h"

/* ---- hashing: FNV-1a carried on, and a splitmix64 stream drawn from a hash ---- */
static unsigned long long t_mix(unsigned long long h, const void *p, size_t n)
{
  for (size_t k = 0; k < n; k++) h = (h ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
  return h;
}
#define MIX(h, v)                           \
  do {                                      \
    const long long mix_v_ = (long long)(v); \
    (h) = t_mix((h), &mix_v_, sizeof(mix_v_)); \
  } while (0)
#define MIX_F(h, v)                         \
  do {                                      \
    const double mix_v_ = (double)(v);      \
    (h) = t_mix((h), &mix_v_, sizeof(mix_v_)); \
  } while (0)

static unsigned long long t_next(unsigned long long *h)
{
  unsigned long long z = (*h += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int t_int(unsigned long long *h, int below) { return (int)(t_next(h) % (unsigned long long)below); }
/* in [-1000, 1000), all 53 bits in use */
static double t_real(unsigned long long *h) { return (double)(t_next(h) >> 11) / 9007199254740992.0 * 2000.0 - 1000.0; }
static double t_real_or_nan(unsigned long long *h) { return t_int(h, 5) == 0 ? (double)NAN : t_real(h); }

/* what every launch of the process has in common: the device that is set, the stream */
static unsigned long long t_call(const char *launcher, hipStream_t s)
{
  unsigned long long h = t_mix(1469598103934665603ull, launcher, strlen(launcher));
  MIX(h, standin_device);
  MIX(h, s != NULL);
  return h;
}

/* ---- the measurement: the records, and the marks that vs_measure has filled with -1 ---- */
hipError_t vs_launch_measure(const VsAcArgs *a, int lds_doubles, hipStream_t s)
{
  unsigned long long call = t_call("measure", s);
  MIX(call, a->pitch);
  MIX(call, a->n_lanes);
  MIX(call, a->n_samples);
  MIX(call, a->marks != NULL);
  MIX(call, a->marks_pitch);
  MIX(call, a->polarity);
  MIX(call, lds_doubles);
  for (long i = 0; i < a->n_lanes; i++) {
    const VsAcRow *r = &a->rows[i];
    const int16_t *x = a->pcm + i * a->pitch;
    unsigned long long h = call;
    MIX(h, i);
    MIX(h, r->len);
    MIX(h, r->fs);
    MIX(h, r->tmin);
    MIX(h, r->tmax);
    CHECK(r->len >= 0 && r->len <= a->n_samples);
    h = t_mix(h, x, (size_t)r->len * sizeof(int16_t));
    h = t_mix(h, x + r->len, (size_t)(a->n_samples - r->len) * sizeof(int16_t)); /* the padding */
    vs_acoustic *o = &a->out[i];
    double *d = &o->f0_hz;
    for (int k = 0; k < 10; k++) d[k] = t_real_or_nan(&h);
    o->p0 = t_int(&h, 2048);
    o->n_periods = t_int(&h, 50) - 1;
    o->first_mark = t_int(&h, 2048);
    o->status = t_int(&h, 3) ? 0 : t_int(&h, 16);
    if (a->marks) {
      int32_t *m = a->marks + i * a->marks_pitch;
      for (long j = 0; j < a->marks_pitch; j++) CHECK(m[j] == -1);
      const long n = t_int(&h, 4) == 0 ? 0 : t_int(&h, (int)a->marks_pitch + 1); /* none; up to a full row */
      int32_t at = 0;
      for (long j = 0; j < n; j++) m[j] = (at += 1 + t_int(&h, 300));
    }
  }
  return hipSuccess;
}

hipError_t vs_launch_glottal(const VsGlArgs *a, hipStream_t s)
{
  unsigned long long call = t_call("glottal", s);
  MIX(call, a->pitch);
  MIX(call, a->n_lanes);
  MIX(call, a->n_samples);
  MIX(call, a->marks_pitch);
  MIX(call, a->cycles != NULL);
  MIX(call, a->cycles_pitch);
  MIX(call, a->level_open);
  MIX(call, a->level_mid);
  MIX(call, a->polarity);
  CHECK(a->meas && a->marks && a->out);
  for (long i = 0; i < a->n_lanes; i++) {
    unsigned long long h = call;
    MIX(h, i);
    h = t_mix(h, &a->meas[i], sizeof(vs_acoustic)); /* what the measurement's stand-in wrote: no padding in it */
    h = t_mix(h, a->marks + i * a->marks_pitch, (size_t)a->marks_pitch * sizeof(int32_t));
    h = t_mix(h, a->pcm + i * a->pitch, (size_t)a->n_samples * sizeof(int16_t));
    vs_glottal_rec *o = &a->out[i];
    double *d = &o->oq;
    const int none = t_int(&h, 5) == 0;
    for (int k = 0; k < 5; k++) d[k] = none ? (double)NAN : t_real_or_nan(&h);
    /* as many cycles as the marks leave room for; now and then one more than the program's array holds */
    o->n_cycles = none ? 0 : t_int(&h, a->marks_pitch - 1);
    o->n_rejected = t_int(&h, 3) == 0 ? a->marks_pitch - 1 - o->n_cycles : 0;
    o->status = t_int(&h, 16);
    o->reserved_ = 0;
    if (a->cycles) {
      vs_glottal_cycle *c = a->cycles + i * a->cycles_pitch;
      for (long j = 0; j < o->n_cycles + o->n_rejected && j < a->cycles_pitch; j++) {
        int32_t *f = &c[j].peak;
        for (int k = 0; k < 12; k++) f[k] = t_int(&h, 40000) - 20000;
      }
    }
  }
  return hipSuccess;
}

/* ---- the frame analyses: a record per frame, its formants, its set ---- */
static void t_frames(const VsLpcArgs *a, unsigned long long call)
{
  MIX(call, a->pitch);
  MIX(call, a->n_lanes);
  MIX(call, a->total_frames);
  MIX(call, a->frames_pitch);
  MIX(call, a->order);
  MIX(call, a->pre);
  MIX(call, a->n_formants);
  MIX_F(call, a->f_lo);
  MIX(call, a->coefs != NULL);
  CHECK(a->frames && (a->formants != NULL) == (a->n_formants != 0));
  const size_t nf = (size_t)a->n_formants, nc = (size_t)a->order + 1;
  long total = 0;
  for (long i = 0; i < a->n_lanes; i++) {
    const VsLpcRow *r = &a->rows[i];
    unsigned long long h = call;
    MIX(h, i);
    MIX(h, r->first);
    MIX(h, r->fs);
    MIX(h, r->L);
    MIX(h, r->H);
    MIX(h, r->s0);
    MIX(h, r->n_frames);
    CHECK(r->first == total && r->n_frames >= 0 && r->n_frames <= a->frames_pitch && r->s0 >= a->pre);
    total += r->n_frames;
    h = t_mix(h, a->windows + r->woff, (size_t)r->L * sizeof(int32_t));
    /* the samples its frames cover, from the one the pre-emphasis reaches back to */
    if (r->n_frames > 0) {
      const long end = (long)r->s0 + (long)(r->n_frames - 1) * r->H + r->L;
      CHECK(end <= a->pitch);
      h = t_mix(h, a->pcm + i * a->pitch, (size_t)end * sizeof(int16_t));
    }
    for (long j = 0; j < r->n_frames; j++) {
      const size_t at = (size_t)i * (size_t)a->frames_pitch + (size_t)j;
      vs_lpc_frame *f = &a->frames[at];
      f->r0 = t_real(&h);
      f->err = t_real_or_nan(&h);
      f->start = r->s0 + (int32_t)j * r->H;
      f->status = t_int(&h, 3) ? 0 : 1 << t_int(&h, 3);
      f->n_formants = f->status ? 0 : t_int(&h, a->n_formants + 1);
      f->reserved_ = 0;
      for (size_t q = 0; q < 2 * nf; q++) a->formants[at * 2 * nf + q] = q < 2 * (size_t)f->n_formants ? t_real(&h) : (double)NAN;
      if (a->coefs)
        for (size_t t = 0; t < nc; t++) a->coefs[at * nc + t] = t ? t_real(&h) / 1000.0 : 1.0;
    }
  }
  CHECK(total == a->total_frames);
}

hipError_t vs_launch_lpc(const VsLpcArgs *a, hipStream_t s)
{
  t_frames(a, t_call("lpc", s));
  return hipSuccess;
}

hipError_t vs_launch_iaif(const VsIaifArgs *a, hipStream_t s)
{
  unsigned long long call = t_call("iaif", s);
  MIX(call, a->glottal_order);
  MIX_F(call, a->leak);
  CHECK(a->glottal == NULL && a->lpc.pre == 0); /* neither program asks for the glottal sets */
  t_frames(&a->lpc, call);
  return hipSuccess;
}

/* ---- the filters: every sample below a row's length, none past it ---- */
static unsigned long long t_filter_call(unsigned long long call, int arith, int mode, long in_pitch, long out_pitch,
                                        long n_lanes, long sets_pitch, int order, int vec_ok, int with_stat)
{
  MIX(call, arith);
  MIX(call, mode);
  MIX(call, in_pitch);
  MIX(call, out_pitch);
  MIX(call, n_lanes);
  MIX(call, sets_pitch);
  MIX(call, order);
  MIX(call, vec_ok);
  MIX(call, with_stat);
  return call;
}
/* n_sets / hop / offset / length lie alike in vs_track_row and vs_inverse_row; f0 and f1 are the two floats behind them */
static unsigned long long t_filter_row(unsigned long long h, long i, const vs_track_row *r, const int16_t *in, int16_t *out,
                                       long out_pitch, const double *sets, int order)
{
  MIX(h, i);
  MIX(h, r->n_sets);
  MIX(h, r->hop);
  MIX(h, r->offset);
  MIX(h, r->length);
  MIX_F(h, r->gain);
  MIX_F(h, r->pre_emphasis);
  CHECK(r->length >= 0 && r->length <= out_pitch && r->n_sets >= 1);
  h = t_mix(h, in, (size_t)r->length * sizeof(int16_t));
  h = t_mix(h, out, (size_t)out_pitch * sizeof(int16_t)); /* what went up as the output row */
  h = t_mix(h, sets, (size_t)r->n_sets * (size_t)(order + 1) * sizeof(double));
  for (long j = 0; j < r->length; j++) out[j] = (int16_t)(t_next(&h) & 0xFFFF);
  return h;
}

hipError_t vs_launch_track(int arith, int mode, const VsTrackArgs *a, hipStream_t s)
{
  const unsigned long long call = t_filter_call(t_call("track", s), arith, mode, a->in_pitch, a->out_pitch, a->n_lanes,
                                                a->sets_pitch, a->order, a->vec_ok, a->stat != NULL);
  CHECK(a->gains == NULL); /* vtrack has no per-set gains */
  for (long i = 0; i < a->n_lanes; i++) {
    unsigned long long h = t_filter_row(call, i, &a->rows[i], a->in + i * a->in_pitch, a->out + i * a->out_pitch,
                                        a->out_pitch, a->coefs + (size_t)i * (size_t)a->sets_pitch * (size_t)(a->order + 1),
                                        a->order);
    if (a->stat) {
      a->stat[i].status = t_int(&h, 4) == 0;
      a->stat[i].n_unusable = t_int(&h, a->rows[i].n_sets + 1);
    }
  }
  return hipSuccess;
}

hipError_t vs_launch_inverse(int arith, int mode, const VsInverseArgs *a, hipStream_t s)
{
  const unsigned long long call = t_filter_call(t_call("inverse", s), arith, mode, a->in_pitch, a->out_pitch, a->n_lanes,
                                                a->sets_pitch, a->order, a->vec_ok, a->stat != NULL);
  for (long i = 0; i < a->n_lanes; i++) {
    const vs_inverse_row *r = &a->rows[i];
    const vs_track_row as_track = {r->n_sets, r->hop, r->offset, r->length, r->scale, r->de_emphasis};
    unsigned long long h = t_filter_row(call, i, &as_track, a->in + i * a->in_pitch, a->out + i * a->out_pitch, a->out_pitch,
                                        a->coefs + (size_t)i * (size_t)a->sets_pitch * (size_t)(a->order + 1), a->order);
    if (a->stat) {
      a->stat[i].status = t_int(&h, 4) == 0;
      a->stat[i].n_unusable = t_int(&h, r->n_sets + 1);
      a->stat[i].n_clipped = t_int(&h, r->length + 1);
      a->stat[i].reserved_ = 0;
    }
  }
  return hipSuccess;
}

/* ---- what vs_api.c links and none of these programs reaches ---- */
hipError_t vs_launch_kernel(int arith, int kind, bool log, bool wave_specialised, bool pre1, const VsKernelArgs *args,
                            unsigned grid, size_t lds_bytes, hipStream_t stream)
{
  return hipErrorUnknown;
}
hipError_t vs_launch_filter_wide(int arith, const VsKernelArgs *args, unsigned grid, hipStream_t stream) { return hipErrorUnknown; }
hipError_t vs_launch_out_noise(const VsKernelArgs *args, hipStream_t stream) { return hipErrorUnknown; }
hipError_t vs_launch_reseed(VsDevLane *lanes, const unsigned long long *seeds, const unsigned long long *out_seeds,
                            int n_lanes, hipStream_t stream)
{
  return hipErrorUnknown;
}
hipError_t vs_launch_selftest(unsigned long long *bad_dev, hipStream_t stream) { return hipErrorUnknown; }
hipError_t vs_launch_simd_probe(int waves, unsigned grid, size_t lds_bytes, unsigned *out_dev, hipStream_t stream)
{
  return hipErrorUnknown;
}
/* of csrc/vs_delivery.c, which is not part of this program: the pool buffers a host-buffer call grows */
void vs_pool_release(vs_ctx *ctx)
{
  if (ctx->pool.d_in) (void)hipFree(ctx->pool.d_in);
  if (ctx->pool.d_aux) (void)hipFree(ctx->pool.d_aux);
  memset(&ctx->pool, 0, sizeof(ctx->pool));
}

/* ---- the program ---- */
#define main cli_main
#include CLI_SOURCE
#undef main

int main(int argc, char **argv)
{
  const char *e = getenv("VS_STANDIN_FAIL_AT");
  fail_at = e ? atoi(e) : 0;
  return cli_main(argc, argv);
}
