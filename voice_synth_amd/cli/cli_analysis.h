/*
 * cli_analysis.h -- what the five analysis programs share beyond cli_common.h: the range helpers of their parsers, the
 * batch of the measuring tools (acoustic, glottal, formants), the lag range by which acoustic and glottal accept a file,
 * the IAIF options of formants and vinverse, the scaffold of the filter tools (vtrack, vinverse).  Each program keeps its
 * usage line, its own letters, its library calls and its printer.
 */
#ifndef VS_CLI_ANALYSIS_H
#define VS_CLI_ANALYSIS_H

#include "cli_common.h"

/* a whole number in [lo, hi] */
static inline int whole(double v, double lo, double hi) { return v == floor(v) && v >= lo && v <= hi; }

/* ---- the measuring tools: all files of a command line as one batch ---- */
typedef struct {
  VsWavRow *rows;  /* the files that were read and accepted, in command-line order */
  int n, bad;      /* bad: some file was not (exit status 2) */
  int32_t maxlen;
  int16_t *pcm;    /* [n][maxlen], each row zero-padded, with its own length and rate */
  int32_t *fs, *len;
} VsCliBatch;

/* Reads every file; accept(row, k, arg) returns 0 for a row that is to be the batch's k-th, or says on stderr why not.
 * 0, or -1 when memory runs out; vs_cli_batch_free either way. */
static inline int vs_cli_batch_load(const char *prog, char **files, int nfiles, int (*accept)(const VsWavRow *, int, void *),
                                    void *arg, VsCliBatch *b)
{
  memset(b, 0, sizeof(*b));
  b->maxlen = 1;
  b->rows = (VsWavRow *)calloc((size_t)nfiles, sizeof(VsWavRow));
  for (int k = 0; b->rows && k < nfiles; k++) {
    VsWavRow *r = &b->rows[b->n];
    if (vs_cli_read_wav(prog, files[k], r) != 0) {
      b->bad = 1;
    } else if (accept(r, b->n, arg) != 0) {
      free(r->x);
      r->x = NULL;
      b->bad = 1;
    } else {
      if (r->len > b->maxlen) b->maxlen = r->len;
      b->n++;
    }
  }
  const size_t n = (size_t)(b->n ? b->n : 1);
  b->pcm = (int16_t *)calloc(n * (size_t)b->maxlen, sizeof(int16_t));
  b->fs = (int32_t *)malloc(n * sizeof(int32_t));
  b->len = (int32_t *)malloc(n * sizeof(int32_t));
  if (!b->rows || !b->pcm || !b->fs || !b->len) {
    fprintf(stderr, "%s: out of memory\n", prog);
    return -1;
  }
  for (int k = 0; k < b->n; k++) {
    memcpy(b->pcm + (size_t)k * b->maxlen, b->rows[k].x, (size_t)b->rows[k].len * sizeof(int16_t));
    b->fs[k] = b->rows[k].fs;
    b->len[k] = b->rows[k].len;
  }
  return 0;
}

static inline void vs_cli_batch_free(VsCliBatch *b)
{
  for (int k = 0; b->rows && k < b->n; k++) free(b->rows[k].x);
  free(b->rows);
  free(b->pcm);
  free(b->fs);
  free(b->len);
  memset(b, 0, sizeof(*b));
}

/* acoustic and glottal: a row is accepted by its lag range tmin..tmax, and the marks' row has room for the longest one's.
 * The range and what vs_measure refuses of it are include/voice_synth.h's formulas ("acoustic measurement"), restated
 * here so that one file's rate is that file's refusal and not the whole call's. */
typedef struct {
  const char *prog;
  const vs_measure_opts *opts;
  int want_marks; /* 0: mpitch stays what it is */
  size_t mpitch;
} VsCliLag;

static inline int vs_cli_lag_accept(const VsWavRow *r, int k, void *arg)
{
  VsCliLag *l = (VsCliLag *)arg;
  const double tmin = floor((double)r->fs / (double)l->opts->f0_max), tmax = ceil((double)r->fs / (double)l->opts->f0_min);
  if (!(r->fs > 0 && tmin >= 2.0 && tmin < tmax && tmax <= VS_AC_MAX_LAG)) {
    fprintf(stderr, "%s: %s: rate %d Hz with F0 %g..%g Hz is outside the measurement's lag range\n", l->prog, r->name,
            (int)r->fs, (double)l->opts->f0_min, (double)l->opts->f0_max);
    return -1;
  }
  const size_t room = (size_t)(r->len / tmin) + 2; /* at most len / tmin + 1 marks, and the -1 behind the last */
  if (l->want_marks && room > l->mpitch) l->mpitch = room;
  return 0;
}

/* ---- -I [-g glottal_order] [-l leak]: formants and vinverse ---- */
typedef struct {
  int on, args; /* -I was given; -g or -l was */
  vs_iaif_opts opts;
} VsCliIaif;

/* the value of -g or -l; 0, or -1 out of range */
static inline int vs_cli_iaif_value(VsCliIaif *s, char letter, double v)
{
  if (letter == 'g' ? !whole(v, 1, VS_MAX_ORDER) : !(v >= 0.0 && v <= 1.0)) return -1;
  if (letter == 'g') s->opts.glottal_order = (int32_t)v;
  else s->opts.leak = v;
  s->args = 1;
  return 0;
}

/* After the parse.  IAIF has no analysis pre-emphasis, and -g and -l need -I: -1.  With -I the frame options go over
 * into s->opts, and *lpc becomes the vs_lpc_opts of the same frames (for vs_lpc_frames and the *_from_lpc rows). */
static inline int vs_cli_iaif_finish(VsCliIaif *s, vs_lpc_opts *lpc)
{
  if ((s->on && lpc->pre_emphasis) || (s->args && !s->on)) return -1;
  if (!s->on) return 0;
  s->opts.order = lpc->order;
  s->opts.window = lpc->window;
  s->opts.n_formants = lpc->n_formants;
  s->opts.window_s = lpc->window_s;
  s->opts.hop_s = lpc->hop_s;
  return vs_iaif_lpc_opts(&s->opts, lpc) == VS_OK ? 0 : -1;
}

/* ---- the filter tools: -i in.wav -o out.wav ( -v id[,id]... | -m model.wav ) [-G] [-t hop_ms] [-O order] ---- */
typedef struct {
  const char *in, *out, *ids, *model;
  int glide;        /* -G */
  vs_lpc_opts opts; /* the analysis of -m: no formants */
  int n_tab, tabs[64];
  VsWavRow src, mod;
} VsCliFilter;

static inline void vs_cli_filter_init(VsCliFilter *f)
{
  memset(f, 0, sizeof(*f));
  vs_lpc_defaults(&f->opts);
  f->opts.n_formants = 0;
}

/* argv[*i]: 1 one of the shared options (*i on its value, if it has one), 0 not one of them, -1 refused */
static inline int vs_cli_filter_arg(VsCliFilter *f, int argc, char **argv, int *i)
{
  const char *a = argv[*i];
  double v = 0.0;
  if (strcmp(a, "-G") == 0) {
    f->glide = 1;
    return 1;
  }
  if (a[0] != '-' || !a[1] || a[2] || !strchr("iovmtO", a[1])) return 0;
  if (*i + 1 >= argc) return -1;
  const char *s = argv[++*i];
  if (a[1] == 'i') f->in = s;
  else if (a[1] == 'o') f->out = s;
  else if (a[1] == 'v') f->ids = s;
  else if (a[1] == 'm') f->model = s;
  else if (!number(s, &v) || (a[1] == 't' ? !(v > 0.0) : !whole(v, 1, VS_MAX_ORDER))) return -1;
  else if (a[1] == 't') f->opts.hop_s = v / 1000.0;
  else f->opts.order = (int32_t)v;
  return 1;
}

/* After the parse: both files, one of -v and -m, and -v's list id[,id]... of at least min_tables known ids.  0 or -1. */
static inline int vs_cli_filter_check(VsCliFilter *f, int min_tables)
{
  if (!f->in || !f->out || (!f->ids == !f->model)) return -1;
  if (!f->ids) return 0;
  for (const char *s = f->ids;;) {
    double A[VS_NCOEF];
    if (!*s || f->n_tab == 64 || vs_vowel_coefficients((unsigned char)*s, A) != VS_OK) return -1;
    f->tabs[f->n_tab++] = (unsigned char)*s++;
    if (!*s) break;
    if (*s++ != ',') return -1;
  }
  return f->n_tab < min_tables ? -1 : 0;
}

/* the input and the model; 0, or 2 with the file named on stderr */
static inline int vs_cli_filter_read(const char *prog, VsCliFilter *f)
{
  if (vs_cli_read_wav(prog, f->in, &f->src) != 0) return 2;
  if (f->model && vs_cli_read_wav(prog, f->model, &f->mod) != 0) return 2;
  if (f->src.len == 0) {
    fprintf(stderr, "%s: %s: no samples\n", prog, f->in);
    return 2;
  }
  return 0;
}

/* -v: the tables' sets [n_tab][VS_NCOEF] (NULL: no memory), and the row's hop: one table holds; more are the anchors of
 * a glide over the N samples with offset 0, the first at sample 0, the last from sample (n_tab - 1) * hop on */
static inline double *vs_cli_filter_tables(const VsCliFilter *f)
{
  double *coefs = (double *)calloc((size_t)f->n_tab * VS_NCOEF, sizeof(double));
  for (int k = 0; coefs && k < f->n_tab; k++) vs_vowel_coefficients(f->tabs[k], coefs + (size_t)k * VS_NCOEF);
  return coefs;
}
static inline int32_t vs_cli_filter_hop(const VsCliFilter *f)
{
  const long hop = f->n_tab > 1 ? ((long)f->src.len - 1) / (long)(f->n_tab - 1) : 1;
  return (int32_t)(hop < 1 ? 1 : hop);
}

/* -m: the model's frame count, 0 where it has none or its rate puts the window out of range (the tool's *_from_lpc row
 * refuses the same); the message for that, and the exit status 2 */
static inline int32_t vs_cli_filter_frames(const VsCliFilter *f)
{
  int32_t nfr = 0;
  return vs_lpc_frames(&f->opts, f->mod.fs, f->mod.len, &nfr) == VS_OK ? nfr : 0;
}
static inline int vs_cli_filter_no_frame(const char *prog, const VsCliFilter *f)
{
  fprintf(stderr, "%s: %s: no analysis frame (%d samples at %d Hz, %g ms window, order %d)\n", prog, f->model,
          (int)f->mod.len, (int)f->mod.fs, f->opts.window_s * 1000.0, (int)f->opts.order);
  return 2;
}

static inline void vs_cli_filter_free(VsCliFilter *f)
{
  free(f->src.x);
  free(f->mod.x);
}

#endif
