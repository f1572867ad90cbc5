/* A STAND-IN HIP runtime for the host code that is tested without a device (tests/c/test_blocks_asan.c,
 * tests/c/test_hostcall_asan.c, tests/c/test_plan_trace.c, tests/c/test_cli_trace.c): one gfx950 device (STANDIN_DEVICES
 * of them where a program defines it; standin_device is the one that is set), device and pinned memory are malloc,
 * streams and events small heap objects, copies memcpy and fills memset, nothing is ever pending.  It counts the calls
 * it gets, can fail the k-th one, and keeps a list of the allocations and one of the copies and fills.  Included once,
 * into the program's one translation unit that holds main. */
#ifndef HIP_STANDIN_H
#define HIP_STANDIN_H

#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("line %d: %s (fail_at %d)\n", __LINE__, #c, fail_at); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

/* ---- the stand-in runtime ---- */
static int calls, fail_at;       /* fail_at: the call that fails (1 = the next one), 0 = none */
static const char *failed_fn;    /* ... its name and, for an event call, its event */
static void *failed_ev;
static int dev_live, pin_live, ev_live, stream_live, pin_allocs, pin_frees, dev_allocs, stream_syncs;

static int failing(const char *fn, void *ev)
{
  if (++calls != fail_at) return 0;
  failed_fn = fn;
  failed_ev = ev;
  return 1;
}
#define MAYFAIL(ev) \
  if (failing(__func__, (void *)(ev))) return hipErrorUnknown

#ifndef STANDIN_DEVICES
#define STANDIN_DEVICES 1
#endif
#ifndef STANDIN_NULL_STREAM /* 1: the code under test works on the null stream (the command-line programs) */
#define STANDIN_NULL_STREAM 0
#endif
static int standin_cu_count = 256; /* what hipGetDeviceProperties reports */
static int standin_device;
hipError_t hipGetDeviceCount(int *n)
{
  *n = STANDIN_DEVICES;
  return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int d)
{
  memset(prop, 0, sizeof(*prop));
  snprintf(prop->name, sizeof(prop->name), "stand-in");
  snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950:sramecc+:xnack-");
  prop->multiProcessorCount = standin_cu_count;
  return d >= 0 && d < STANDIN_DEVICES ? hipSuccess : hipErrorInvalidDevice;
}
hipError_t hipDeviceGetPCIBusId(char *id, int len, int d)
{
  snprintf(id, (size_t)len, "0000:00:00.0");
  return hipSuccess;
}
hipError_t hipSetDevice(int d)
{
  MAYFAIL(NULL);
  if (d < 0 || d >= STANDIN_DEVICES) return hipErrorInvalidDevice;
  standin_device = d;
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
  MAYFAIL(NULL);
  *s = (hipStream_t)malloc(1);
  stream_live++;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
  free(s);
  stream_live--;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
  stream_syncs++;
  MAYFAIL(NULL);
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags)
{
  MAYFAIL(e);
  return *(char *)e ? hipSuccess : hipErrorInvalidHandle; /* the library only ever waits for an event it has recorded */
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
  MAYFAIL(NULL);
  *e = (hipEvent_t)calloc(1, 1); /* the byte: recorded */
  ev_live++;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
  MAYFAIL(a);
  *ms = 0.0f;
  return *(char *)a && *(char *)b ? hipSuccess : hipErrorInvalidHandle;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
  MAYFAIL(e);
  *(char *)e = 1;
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
  MAYFAIL(e);
  (void)*(volatile char *)e; /* reads the event, so that ASan sees a destroyed one */
  return hipSuccess;
}
/* what gives something back does so even when it is the call that "fails": the library cannot do anything about it */
hipError_t hipEventDestroy(hipEvent_t e)
{
  free(e);
  ev_live--;
  MAYFAIL(NULL);
  return hipSuccess;
}
/* every allocation, in order: 'd' device, 'p' pinned; a pointer into a live one can be named "allocation k + offset".
 * With STANDIN_FILL defined a new block is filled with that byte, so that what a program copies out of one is the same
 * in every run */
typedef struct StandinAlloc {
  char kind;
  int live;
  size_t bytes;
  const char *ptr;
} StandinAlloc;
#ifndef STANDIN_ALLOC_LOG
#define STANDIN_ALLOC_LOG 64
#endif
static StandinAlloc alloc_log[STANDIN_ALLOC_LOG];
static int n_allocs;
static void *standin_alloc(char kind, size_t n)
{
  void *p = malloc(n);
#ifdef STANDIN_FILL
  if (p) memset(p, STANDIN_FILL, n);
#endif
  if (n_allocs < STANDIN_ALLOC_LOG) alloc_log[n_allocs] = (StandinAlloc){kind, 1, n, (const char *)p};
  n_allocs++;
  return p;
}
static void standin_release(void *p)
{
  for (int k = 0; k < n_allocs && k < STANDIN_ALLOC_LOG; k++)
    if (alloc_log[k].live && alloc_log[k].ptr == (const char *)p) alloc_log[k].live = 0;
  free(p);
}
/* the live allocation p points into (-1: none of the list's), and how far */
static int standin_find(const void *p, size_t *off)
{
  for (int k = 0; k < n_allocs && k < STANDIN_ALLOC_LOG; k++) {
    const StandinAlloc *a = &alloc_log[k];
    if (a->live && (const char *)p >= a->ptr && (const char *)p < a->ptr + (a->bytes ? a->bytes : 1)) {
      *off = (size_t)((const char *)p - a->ptr);
      return k;
    }
  }
  return -1;
}
hipError_t hipMalloc(void **p, size_t n)
{
  MAYFAIL(NULL);
  *p = standin_alloc('d', n);
  dev_live++;
  dev_allocs++;
  return hipSuccess;
}
hipError_t hipFree(void *p)
{
  if (p) dev_live--;
  standin_release(p);
  MAYFAIL(NULL);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags)
{
  MAYFAIL(NULL);
  *p = standin_alloc('p', n);
  pin_live++;
  pin_allocs++;
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned flags)
{
  MAYFAIL(NULL);
  *dev = host; /* mapped memory: the device sees the block itself */
  return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
  if (p) pin_live--, pin_frees++;
  standin_release(p);
  MAYFAIL(NULL);
  return hipSuccess;
}
/* every copy and fill that was not the failing call, in order: 'U' up, 'D' down, 'F' fill; dev = its device side, also as
 * allocation + offset (the block may be gone when the list is read); hash: FNV-1a over the bytes that moved */
typedef struct StandinCopy {
  char kind;
  size_t bytes;
  const void *dev;
  hipStream_t stream;
  int alloc;
  size_t off;
  unsigned long long hash;
} StandinCopy;
#ifndef STANDIN_COPY_LOG
#define STANDIN_COPY_LOG 64
#endif
static StandinCopy copy_log[STANDIN_COPY_LOG];
static int n_copies;
static unsigned long long standin_hash(const void *p, size_t n)
{
  unsigned long long h = 1469598103934665603ull;
  for (size_t k = 0; k < n; k++) h = (h ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
  return h;
}
static void log_copy(char kind, size_t bytes, const void *dev, hipStream_t s)
{
  if (n_copies < STANDIN_COPY_LOG) {
    StandinCopy *c = &copy_log[n_copies];
    *c = (StandinCopy){kind, bytes, dev, s, -1, 0, standin_hash(dev, bytes)};
    c->alloc = standin_find(dev, &c->off);
  }
  n_copies++;
}
#ifndef STANDIN_COPY_DOWN /* the record upload only ever copies up */
#define STANDIN_COPY_DOWN 0
#endif
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
  MAYFAIL(NULL);
  memcpy(dst, src, n);
  const int down = STANDIN_COPY_DOWN && kind == hipMemcpyDeviceToHost;
  log_copy(down ? 'D' : 'U', n, down ? src : dst, s);
  /* never on the null stream, unless that is where the code under test works */
  return (kind == hipMemcpyHostToDevice || down) && (s || STANDIN_NULL_STREAM) ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t s)
{
  MAYFAIL(NULL);
  memset(dst, value, n);
  log_copy('F', n, dst, s);
  return s || STANDIN_NULL_STREAM ? hipSuccess : hipErrorInvalidValue;
}

#endif
