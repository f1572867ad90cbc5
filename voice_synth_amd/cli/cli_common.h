/*
 * cli_common.h -- shared bits of the command-line programs.
 *
 * The programs keep the reference's argv, stdout text, exit codes and .wav layout
 *  and do all sample computation through include/voice_synth.h on the
 * GPU.  Environment (additions; the reference has no such knobs):
 *   VS_SEED        Philox key of the draw stream (default: time(NULL), like srandom(time(NULL)))
 *   VS_WAV_HEADER  44 (default, the ILP32 layout the reference documents) or 72 (what an LP64
 *                  build of the reference writes and reads)
 *   VS_DEVICE      HIP device ordinal (default 0)
 *   VS_ARITH       "exact" (default) or "fma"
 */
#ifndef VS_CLI_COMMON_H
#define VS_CLI_COMMON_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "voice_synth.h"

static inline int vs_cli_header_bytes(void)
{
  const char *e = getenv("VS_WAV_HEADER");
  if (e && atoi(e) == 72) return 72;
  return 44;
}

static inline uint64_t vs_cli_seed(void)
{
  const char *e = getenv("VS_SEED");
  if (e && *e) return (uint64_t)strtoull(e, NULL, 0);
  return (uint64_t)time(NULL);
}

static inline int vs_cli_open_ctx(vs_ctx **ctx)
{
  const char *d = getenv("VS_DEVICE");
  int rc = vs_ctx_create(d ? atoi(d) : 0, ctx);
  if (rc != VS_OK) {
    fprintf(stderr, "voice_synth: cannot open GPU device: %s\n", vs_strerror(rc));
    return rc;
  }
  const char *a = getenv("VS_ARITH");
  if (a && strcmp(a, "fma") == 0) vs_ctx_set_arith(*ctx, VS_ARITH_FMA);
  return VS_OK;
}

/* a whole argument that is a number: "inf" and "1e999" are */
static inline int vs_cli_real(const char *s, double *v)
{
  char *end = NULL;
  *v = strtod(s, &end);
  return end && end != s && !*end;
}
/* ... and finite */
static inline int number(const char *s, double *v) { return vs_cli_real(s, v) && isfinite(*v); }

/* A 16-bit PCM .wav file read whole (the analysis programs), with its header as it stands in the file. */
typedef struct {
  const char *name;
  int16_t *x;
  int32_t len, fs;
  unsigned char header[72];
  int hbytes;
} VsWavRow;

/* 0 on success; else a message "PROG: PATH: ..." on stderr */
static inline int vs_cli_read_wav(const char *prog, const char *path, VsWavRow *r)
{
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "%s: %s: cannot open\n", prog, path);
    return -1;
  }
  const size_t got = fread(r->header, 1, sizeof(r->header), f);
  int32_t fs = 0;
  int tag = 0, bits = 0;
  uint64_t data_bytes = 0;
  const int hbytes = vs_wav_header_read(r->header, got, &fs, &tag, &bits, &data_bytes);
  if (hbytes < 0) {
    fprintf(stderr, "%s: %s: not a .wav file or truncated header\n", prog, path);
    fclose(f);
    return -1;
  }
  if (tag != 1 || bits != 16) {
    fprintf(stderr, "%s: %s: not 16-bit PCM (format tag %d, %d bits per sample)\n", prog, path, tag, bits);
    fclose(f);
    return -1;
  }
  /* payload: everything after the header, in whole samples (as vowel reads it) */
  if (fseek(f, 0, SEEK_END) != 0) {
    fclose(f);
    return -1;
  }
  const long fsize = ftell(f);
  const size_t n = (fsize > hbytes) ? (size_t)(fsize - hbytes) / sizeof(int16_t) : 0;
  if (n > 0x7FFFFFFF) {
    fprintf(stderr, "%s: %s: too long\n", prog, path);
    fclose(f);
    return -1;
  }
  fseek(f, hbytes, SEEK_SET);
  r->x = (int16_t *)malloc((n ? n : 1) * sizeof(int16_t));
  if (!r->x || fread(r->x, sizeof(int16_t), n, f) != n) {
    fprintf(stderr, "%s: %s: read error\n", prog, path);
    free(r->x);
    r->x = NULL;
    fclose(f);
    return -1;
  }
  fclose(f);
  r->name = path;
  r->len = (int32_t)n;
  r->fs = fs;
  r->hbytes = hbytes;
  return 0;
}

/* row's header verbatim (as vowel copies its input's), then n samples; 0, or "PROG: PATH: cannot write" on stderr */
static inline int vs_cli_write_wav(const char *prog, const char *path, const VsWavRow *row, const int16_t *samples, size_t n)
{
  FILE *f = fopen(path, "wb");
  const int ok = f && fwrite(row->header, (size_t)row->hbytes, 1, f) == 1 && fwrite(samples, sizeof(int16_t), n, f) == n;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "%s: %s: cannot write\n", prog, path);
  return ok ? 0 : -1;
}

#endif
