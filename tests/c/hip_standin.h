/* A STAND-IN HIP runtime for the host code that is tested without a device (tests/c/test_blocks_asan.c,
 * tests/c/test_hostcall_asan.c): device and pinned memory are malloc, streams and events small heap objects, copies
 * memcpy and fills memset, nothing is ever pending.  It counts the calls it gets, can fail the k-th one, and keeps a
 * list of the copies and fills.  Included once, into the program's one translation unit that holds main. */
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

hipError_t hipSetDevice(int d)
{
  MAYFAIL(NULL);
  return d == 0 ? hipSuccess : hipErrorInvalidDevice;
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
hipError_t hipMalloc(void **p, size_t n)
{
  MAYFAIL(NULL);
  *p = malloc(n);
  dev_live++;
  dev_allocs++;
  return hipSuccess;
}
hipError_t hipFree(void *p)
{
  if (p) dev_live--;
  free(p);
  MAYFAIL(NULL);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned flags)
{
  MAYFAIL(NULL);
  *p = malloc(n);
  pin_live++;
  pin_allocs++;
  return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
  if (p) pin_live--, pin_frees++;
  free(p);
  MAYFAIL(NULL);
  return hipSuccess;
}
/* every copy and fill that was not the failing call, in order: 'U' up, 'D' down, 'F' fill; dev = its device side */
typedef struct StandinCopy {
  char kind;
  size_t bytes;
  const void *dev;
  hipStream_t stream;
} StandinCopy;
#define STANDIN_COPY_LOG 64
static StandinCopy copy_log[STANDIN_COPY_LOG];
static int n_copies;
static void log_copy(char kind, size_t bytes, const void *dev, hipStream_t s)
{
  if (n_copies < STANDIN_COPY_LOG) copy_log[n_copies] = (StandinCopy){kind, bytes, dev, s};
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
  return (kind == hipMemcpyHostToDevice || down) && s ? hipSuccess : hipErrorInvalidValue; /* never on the null stream */
}
hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t s)
{
  MAYFAIL(NULL);
  memset(dst, value, n);
  log_copy('F', n, dst, s);
  return s ? hipSuccess : hipErrorInvalidValue;
}

#endif
