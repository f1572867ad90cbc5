/*
 * vs_api.c -- host side of the C ABI (include/voice_synth.h): device context, plans
 * (parameter expansion + cos tables + upload) and launches.  C11 + pthreads, the HIP runtime through
 * its C API; the kernels are launched through the extern "C" launchers of vs_kernels.hip.
 *
 * The device-free half of plan creation (lane expansion with the reference's operand types, the order of the lanes, the
 * tables, the launch shape, the knobs of a launch, the layout of the plan's blocks) is csrc/vs_planhost.c: nothing is
 * decided here, this file allocates, uploads and launches what that one says.
 * This translation unit is compiled with -ffp-contract=off.
 */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "vs_internal.h"

double vs_now_ms(void)
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
}

/* Experiments only (tools/gpu_sweep.sh): with VS_DEBUG_TUNING=1 in the environment the knobs
 * are read ONCE, by vs_ctx_create, and go through the same validation as vs_ctx_set_tuning().  Without it
 * no environment variable can change what the library launches. */
static int debug_tuning_from_env(vs_ctx *ctx)
{
  const char *dbg = getenv("VS_DEBUG_TUNING");
  if (!dbg || strcmp(dbg, "1") != 0) return VS_OK;
  vs_tuning t;
  memset(&t, 0, sizeof(t));
  const char *v;
  if ((v = getenv("VS_KERNEL")) != NULL) t.kernel = strcmp(v, "ws") == 0 ? VS_KERNEL_WS : (strcmp(v, "single") == 0 ? VS_KERNEL_SINGLE : VS_KERNEL_AUTO);
  if ((v = getenv("VS_RING_SLOTS")) != NULL) t.ring_slots = atoi(v);
  if ((v = getenv("VS_READY_MIN")) != NULL) t.ready_min = atoi(v);
  if ((v = getenv("VS_WS_PAIRS")) != NULL) t.ws_pairs = atoi(v);
  if ((v = getenv("VS_WS_ROLES")) != NULL) t.ws_roles = atoi(v);
  if ((v = getenv("VS_GEN_LOW")) != NULL) t.gen_low = atoi(v);
  if ((v = getenv("VS_GEN_MIN")) != NULL) t.gen_min = atoi(v);
  if ((v = getenv("VS_MIXED_RINGS")) != NULL) t.mixed_rings = (atoi(v) == 0) ? -1 : (atoi(v) == 1 ? 0 : atoi(v));
  if ((v = getenv("VS_WS_PRIO")) != NULL) t.ws_filter_prio = (atoi(v) == 0) ? -1 : atoi(v);
  return vs_ctx_set_tuning(ctx, &t) == VS_OK ? VS_OK : VS_ERR_ARG;
}

int vs_ctx_create(int device, vs_ctx **out)
{
  if (!out) return VS_ERR_ARG;
  *out = NULL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return VS_ERR_NODEVICE;
  if (device < 0 || device >= count) return VS_ERR_NODEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return VS_ERR_NODEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return VS_ERR_NODEVICE; /* code object is gfx950 only */
  if (hipSetDevice(device) != hipSuccess) return VS_ERR_NODEVICE;
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(vs_ctx));
  if (!ctx) return VS_ERR_NOMEM;
  ctx->device = device;
  ctx->arith = VS_ARITH_EXACT;
  ctx->stream = NULL;
  ctx->upload = NULL;
  ctx->last_hip_error = 0;
  snprintf(ctx->name, sizeof(ctx->name), "%.80s (%.40s)", prop.name, prop.gcnArchName);
  ctx->cu_count = prop.multiProcessorCount;
  memset(&ctx->tuning, 0, sizeof(ctx->tuning));
  memset(&ctx->pool, 0, sizeof(ctx->pool));
  if (debug_tuning_from_env(ctx) != VS_OK) {
    free(ctx);
    return VS_ERR_ARG;
  }
  *out = ctx;
  return VS_OK;
}

/* The HIP runtime sets up its copy path (staging buffers, the transfer queue of this device) at a process's first
 * host-to-device copy: 27 ms on a bare process whatever the size (tools/hip_startup_probe.c), ~100 ms in one that
 * has loaded PyTorch (profiles/r04_plan_cost.txt).  Paid HERE, once per context, the first time a plan that copies
 * is made and before that plan's clock starts -- so that a first vs_plan_create costs what every later one costs --
 * and NOT by vs_ctx_create: the drop-in programs make zero-copy plans only (VS_PLAN_ZERO_COPY) and never copy. */
int vs_copy_path_warm(vs_ctx *ctx)
{
  if (ctx->copy_warm) return VS_OK;
  const double t0 = vs_now_ms();
  void *scratch = NULL;
  const size_t warm_bytes = 1u << 20;
  void *host = malloc(warm_bytes);
  hipError_t e = host ? hipSetDevice(ctx->device) : hipErrorOutOfMemory;
  /* on the stream the records of later plans go up on (creating a stream costs milliseconds the first time: vs_own_upload) */
  if (e == hipSuccess) e = vs_own_upload(ctx);
  if (e == hipSuccess) e = hipMalloc(&scratch, warm_bytes);
  if (e == hipSuccess) {
    memset(host, 0, warm_bytes);
    e = hipMemcpyAsync(scratch, host, warm_bytes, hipMemcpyHostToDevice, ctx->own_upload);
    if (e == hipSuccess) e = hipMemcpyAsync(host, scratch, sizeof(int), hipMemcpyDeviceToHost, ctx->own_upload);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->own_upload);
    (void)hipFree(scratch);
  }
  free(host);
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return (e == hipErrorOutOfMemory) ? VS_ERR_NOMEM : VS_ERR_HIP;
  }
  ctx->copy_warm = 1;
  ctx->copy_warm_ms = vs_now_ms() - t0;
  return VS_OK;
}

int vs_ctx_set_tuning(vs_ctx *ctx, const vs_tuning *t)
{
  if (!ctx) return VS_ERR_ARG;
  if (!t) {
    memset(&ctx->tuning, 0, sizeof(ctx->tuning));
    return VS_OK;
  }
  if (t->kernel != VS_KERNEL_AUTO && t->kernel != VS_KERNEL_SINGLE && t->kernel != VS_KERNEL_WS) return VS_ERR_ARG;
  if (t->ring_slots < 0 || t->ring_slots > 65536) return VS_ERR_ARG;
  if (t->ready_min < 0 || t->ready_min > 64) return VS_ERR_ARG;
  if (t->ws_pairs < 0 || t->ws_pairs == 3 || t->ws_pairs > 4) return VS_ERR_ARG;
  /* a lane short of gen_low samples starts a round at once: below one super-step the filter wave
   * could starve while the generator waits for company */
  if (t->gen_low != 0 && t->gen_low < VS_SS) return VS_ERR_ARG;
  if (t->gen_min < 0 || t->gen_min > 64) return VS_ERR_ARG;
  if (t->spin_limit < 0) return VS_ERR_ARG;
  if (t->fault < 0 || t->fault > VS_FAULT_REROUND) return VS_ERR_ARG;
  if (t->ws_filter_prio < -1 || t->ws_filter_prio > 3) return VS_ERR_ARG;
  if (t->ws_roles != 0 && t->ws_roles != 2 && t->ws_roles != 3) return VS_ERR_ARG;
  if (t->mixed_rings < -1 || t->mixed_rings > 4096) return VS_ERR_ARG;
  ctx->tuning = *t;
  return VS_OK;
}

void vs_ctx_destroy(vs_ctx *ctx)
{
  if (!ctx) return;
  vs_pool_release(ctx);
  vs_rec_release(ctx, &ctx->rec_measure); /* (they wait for their last copy on own_upload) */
  vs_rec_release(ctx, &ctx->rec_lpc);
  vs_rec_release(ctx, &ctx->rec_track);
  vs_rec_release(ctx, &ctx->rec_inverse);
  vs_rec_release(ctx, &ctx->rec_iaif);
  vs_rec_release(ctx, &ctx->rec_cplpc);
  vs_rec_release(ctx, &ctx->rec_pitch);
  vs_rec_release(ctx, &ctx->rec_guided);
  vs_rec_release(ctx, &ctx->rec_strack);
  vs_rec_release(ctx, &ctx->rec_psola);
  vs_rec_release(ctx, &ctx->rec_psola_ts);
  if (ctx->own_upload) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamDestroy(ctx->own_upload);
  }
  vs_plan_cache_release(ctx);
  for (int k = 0; k < 2; k++)
    if (ctx->timer[k]) (void)hipEventDestroy(ctx->timer[k]);
  vs_planws_destroy(ctx->planws);
  if (ctx->plan_pin) (void)hipHostFree(ctx->plan_pin);
  free(ctx);
}

int vs_ctx_set_stream(vs_ctx *ctx, void *hip_stream)
{
  if (!ctx) return VS_ERR_ARG;
  ctx->stream = (hipStream_t)hip_stream;
  return VS_OK;
}

int vs_ctx_set_arith(vs_ctx *ctx, int arith)
{
  if (!ctx || (arith != VS_ARITH_EXACT && arith != VS_ARITH_FMA && arith != VS_ARITH_F32)) return VS_ERR_ARG;
  ctx->arith = arith;
  return VS_OK;
}

int vs_ctx_last_hip_error(const vs_ctx *ctx) { return ctx ? ctx->last_hip_error : 0; }

int vs_ctx_device_info(const vs_ctx *ctx, char *name, size_t name_len, int *cu_count)
{
  if (!ctx) return VS_ERR_ARG;
  if (name && name_len) snprintf(name, name_len, "%s", ctx->name);
  if (cu_count) *cu_count = ctx->cu_count;
  return VS_OK;
}

int vs_ctx_device_pci(const vs_ctx *ctx, char *bus_id, size_t len)
{
  if (!ctx || !bus_id || len < 16) return VS_ERR_ARG;
  bus_id[0] = '\0';
  const hipError_t e = hipDeviceGetPCIBusId(bus_id, (int)len, ctx->device);
  if (e != hipSuccess) return VS_ERR_HIP;
  return VS_OK;
}

int vs_ctx_synchronize(vs_ctx *ctx)
{
  if (!ctx) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}

int vs_ctx_timer_mark(vs_ctx *ctx, int which)
{
  if (!ctx || (which != 0 && which != 1)) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->timer[which]) VS_HIP(ctx, hipEventCreate(&ctx->timer[which]));
  VS_HIP(ctx, hipEventRecord(ctx->timer[which], ctx->stream));
  return VS_OK;
}

int vs_ctx_timer_elapsed(vs_ctx *ctx, double *ms)
{
  if (!ctx || !ms || !ctx->timer[0] || !ctx->timer[1]) return VS_ERR_ARG;
  float f = 0.0f;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipEventSynchronize(ctx->timer[1]));
  VS_HIP(ctx, hipEventElapsedTime(&f, ctx->timer[0], ctx->timer[1]));
  *ms = (double)f;
  return VS_OK;
}

/* One probe launch per workgroup size: a workgroup per CU (most of the LDS each, like the fused launches), every
 * wavefront reports its HW_ID; "cyclic" = in every workgroup the first four wavefronts run on four different SIMDs
 * and wavefront w runs where wavefront w % 4 does. */
static int simd_probe(vs_ctx *ctx)
{
  if (ctx->simd_probed) return ctx->simd_probed > 0 ? VS_OK : VS_ERR_HIP;
  const unsigned grid = (unsigned)(ctx->cu_count > 0 ? ctx->cu_count : 256);
  unsigned *d = NULL, *h = (unsigned *)calloc((size_t)grid * 16, sizeof(unsigned));
  ctx->simd_probed = -1;
  ctx->simd_cyclic12 = ctx->simd_cyclic8 = 0;
  ctx->simd_odd_wgs = 0;
  if (!h) return VS_ERR_NOMEM;
  hipError_t e = hipSetDevice(ctx->device);
  /* on the context's own non-blocking stream, not the caller's launch stream: the first plan that wants a three-role
   * layout may be made while a kernel of the caller's runs there (the probe still needs the CUs: it starts when they are
   * free, but it does not make vs_plan_create wait for work that was queued behind that kernel) */
  if (e == hipSuccess) e = vs_own_upload(ctx);
  hipStream_t ps = ctx->own_upload;
  if (e == hipSuccess) e = hipMalloc((void **)&d, (size_t)grid * 16 * sizeof(unsigned));
  int ok[2] = {1, 1};
  unsigned odd = 0;
  for (int pass = 0; pass < 2 && e == hipSuccess; pass++) {
    const int waves = pass == 0 ? 12 : 8;
    memset(h, 0, (size_t)grid * 16 * sizeof(unsigned));
    e = hipMemcpyAsync(d, h, (size_t)grid * 16 * sizeof(unsigned), hipMemcpyHostToDevice, ps);
    if (e == hipSuccess) e = vs_launch_simd_probe(waves, grid, (size_t)VS_LDS_LIMIT - 8192, d, ps);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, (size_t)grid * 16 * sizeof(unsigned), hipMemcpyDeviceToHost, ps);
    if (e == hipSuccess) e = hipStreamSynchronize(ps);
    if (e != hipSuccess) break;
    for (unsigned g = 0; g < grid; g++) {
      /* "dealt four at a time": the first four wavefronts land on four DIFFERENT SIMDs (in whatever order -- MI355X
       * shows four rotations of (0, 2, 1, 3)) and wavefront w joins wavefront w % 4, on the same CU */
      int good = 1;
      unsigned seen = 0;
      for (int w = 0; w < waves; w++) {
        const unsigned hw = h[(size_t)g * 16 + (size_t)w], first = h[(size_t)g * 16 + (size_t)(w & 3)];
        if (!(hw & 0x80000000u)) good = 0;
        if (w < 4) seen |= 1u << ((hw >> 4) & 3u);
        else if (((hw >> 4) & 3u) != ((first >> 4) & 3u) || ((hw >> 8) & 0xFFu) != ((first >> 8) & 0xFFu)) good = 0;
      }
      if (seen != 0xFu) good = 0;
      if (!good) {
        ok[pass] = 0;
        odd++;
      }
    }
  }
  if (d) (void)hipFree(d);
  free(h);
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return VS_ERR_HIP;
  }
  ctx->simd_cyclic12 = ok[0];
  ctx->simd_cyclic8 = ok[1];
  ctx->simd_odd_wgs = odd;
  ctx->simd_probed = 1;
  return VS_OK;
}

int vs_ctx_simd_dealing(vs_ctx *ctx, int *cyclic12, int *cyclic8)
{
  if (!ctx) return VS_ERR_ARG;
  const int rc = simd_probe(ctx);
  if (cyclic12) *cyclic12 = ctx->simd_cyclic12;
  if (cyclic8) *cyclic8 = ctx->simd_cyclic8;
  return rc;
}

int vs_ctx_selftest(vs_ctx *ctx, uint64_t *failures)
{
  if (!ctx) return VS_ERR_ARG;
  unsigned long long *d = NULL, h[VS_SELFTEST_COUNTERS] = {0};
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipMalloc((void **)&d, sizeof(h)));
  hipError_t e = hipMemsetAsync(d, 0, sizeof(h), ctx->stream);
  if (e == hipSuccess) e = vs_launch_selftest(d, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return VS_ERR_HIP;
  }
  /* [6]: workgroups of the wave-to-SIMD probe that were not dealt four at a time (all of them if the probe failed) */
  h[6] = (simd_probe(ctx) == VS_OK) ? ctx->simd_odd_wgs : 1ull;
  unsigned long long any = 0;
  for (int k = 0; k < VS_SELFTEST_COUNTERS; k++) {
    if (failures) failures[k] = h[k];
    any |= h[k];
  }
  return any ? VS_ERR_INTERNAL : VS_OK;
}

int vs_dev_alloc(vs_ctx *ctx, size_t bytes, void **ptr)
{
  if (!ctx || !ptr) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipMalloc(ptr, bytes ? bytes : 1));
  return VS_OK;
}
int vs_dev_free(vs_ctx *ctx, void *ptr)
{
  if (!ctx) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipFree(ptr));
  return VS_OK;
}
int vs_dev_upload(vs_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
  if (!ctx) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}
int vs_dev_download(vs_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
  if (!ctx) return VS_ERR_ARG;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}

/* Page-locked host memory for what a big plan sends to the device.  From pageable memory the runtime copies with a
 * kernel of its own, and that kernel waits until the chip has room -- i.e. until the launch before it has ENDED, when
 * that launch fills every CU for its whole duration as the fused kernel does: the plan of batch k + 1 then goes up
 * behind kernel k instead of next to it (bench.py fresh_batches: upload 1.8 ms instead of 0.3).  From page-locked memory
 * it is a DMA transfer. */
static void *plan_pinned_alloc(void *user, size_t bytes)
{
  vs_ctx *ctx = (vs_ctx *)user;
  void *p = NULL;
  if (hipSetDevice(ctx->device) != hipSuccess) return NULL;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return NULL;
  return p;
}
static void plan_pinned_free(void *user, void *ptr)
{
  (void)user;
  if (ptr) (void)hipHostFree(ptr);
}

/* vs_plan_shape's question to the hardware: simd_probe, once per context */
static int plan_dealt(void *user, int waves)
{
  vs_ctx *ctx = (vs_ctx *)user;
  return simd_probe(ctx) == VS_OK && (waves == 12 ? ctx->simd_cyclic12 : ctx->simd_cyclic8);
}

/* The small parts of a plan that copies -- cos rows + tap table, the mixed-rings table, the error word -- share ONE device
 * block that is never smaller than VS_SMALL_BLOCK_MIN and goes up in ONE copy: the runtime moves copies of up to 16 KiB
 * with a kernel of its own, and that kernel waits until the chip has room, i.e. until a fused launch that is running has
 * ENDED (it fills every CU for its whole duration), while a copy of 64 KiB is a DMA transfer that runs next to it --
 * 0.03 ms instead of 2.2 behind a launch (tools/overlap_probe.py, profiles/r05_plan_cost.txt).  Staged in the context's
 * page-locked block, or in *tmp (the caller frees it) when there is none to be had.
 * (the error word is zeroed by the copy, not by hipMemsetAsync: a process's first memset loads the runtime's fill kernel, 20 ms) */
static hipError_t small_block_upload(vs_ctx *ctx, vs_plan *p, const VsPlanLayout *b, const VsPlanTables *tab,
                                     const VsGroupSlot *gmap, hipStream_t up, void **tmp)
{
  if (ctx->plan_pin_bytes < b->small_bytes) {
    if (ctx->plan_pin) (void)hipHostFree(ctx->plan_pin);
    ctx->plan_pin = NULL;
    ctx->plan_pin_bytes = 0;
    if (hipHostMalloc(&ctx->plan_pin, 2 * b->small_bytes, hipHostMallocDefault) == hipSuccess) ctx->plan_pin_bytes = 2 * b->small_bytes;
    else ctx->plan_pin = NULL;
  }
  char *blk = (char *)ctx->plan_pin;
  if (!blk) blk = (char *)(*tmp = calloc(1, b->small_bytes)); /* no page-locked memory: a pageable block of the same size */
  if (!blk) return hipErrorOutOfMemory;
  if (b->cos_bytes) memcpy(blk, tab->costab, b->cos_bytes);
  if (b->gmap_bytes) memcpy(blk + b->small_off_gmap, gmap, b->gmap_bytes);
  memset(blk + b->small_off_err, 0, 64);
  return hipMemcpyAsync(p->d_small, blk, b->small_bytes, hipMemcpyHostToDevice, up);
}

int vs_plan_create_impl(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                        int mode, vs_plan **out)
{
  const int filter_only = (mode & VS_PLAN_FILTER_ONLY) ? 1 : 0;
  const int zero_copy = (mode & VS_PLAN_ZERO_COPY) ? 1 : 0;
  if (!ctx || !lanes || !out || n_lanes == 0 || n_samples == 0) return VS_ERR_ARG;
  if (n_lanes > (size_t)0x7FFFFFC0 || n_samples > (size_t)0x7FFFFF00) return VS_ERR_UNSUPPORTED;
  *out = NULL;
  if (!zero_copy) {
    const int wrc = vs_copy_path_warm(ctx);
    if (wrc != VS_OK) return wrc;
  }
  /* the records are made in the context's plan workspace (csrc/vs_planhost.c: worker threads that sleep between plans,
   * record buffers that are kept -- a fresh 8 MB block per plan is two thousand page faults); everything else of this
   * call is released at `done` */
  if (!ctx->planws) {
    ctx->planws = vs_planws_create();
    vs_planws_set_big_allocator(ctx->planws, plan_pinned_alloc, plan_pinned_free, ctx);
  }
  if (!ctx->planws) return VS_ERR_NOMEM;
  VsDevLane *dl = NULL;
  VsPlanTables tab = {0}; /* cos rows + taps, a wide plan's 40 taps per record */
  VsPlanShape sh = {0};   /* (its gmap: the mixed-rings table) */
  VsPlanLayout b;
  void *small_tmp = NULL; /* stand-in for the page-locked staging block when there is none */
  vs_plan *p = NULL;
  const double t_host0 = vs_now_ms();
  /* Wavefronts are formed from lanes with similar periods: a generator round costs as much as its longest lane and
   * the cos rows of a wavefront are staged once per distinct T2, so a batch with an F0 sweep (BASELINE config 5) is
   * put in the order of (P, T2, options) before it is cut into groups of 64 (vs_expand_all_ordered_ws: one parallel
   * pass makes the records, a batch whose keys differ is then sorted and gathered).  Placement is internal: each lane
   * still writes its own output row (VsDevLane.row), and a lane's result does not depend on its neighbours.  Stable, so
   * homogeneous batches keep their order. */
  VsBatchStats st; /* gathered by the threads that make the records: no walk over all of them per question */
  int rc = vs_expand_all_ordered_ws(ctx->planws, lanes, n_lanes, filter_only, &dl, NULL, &st);
  if (rc == VS_OK) rc = vs_plan_tables_build(lanes, dl, n_lanes, &st, filter_only, &tab);
  if (rc == VS_OK)
    rc = vs_plan_shape(dl, n_lanes, n_samples, &st, filter_only, ctx->cu_count, &ctx->tuning, tab.ltab_entries, plan_dealt, ctx, &sh);
  if (rc == VS_OK && !(p = (vs_plan *)calloc(1, sizeof(vs_plan)))) rc = VS_ERR_NOMEM;
  if (rc != VS_OK) goto done;
  p->ctx = ctx;
  p->n_lanes = n_lanes;
  p->n_samples = n_samples;
  p->shape = sh;
  p->shape.gmap = NULL; /* (released below; the plan keeps the table on the device) */
  p->filter_only = filter_only;
  p->tuning = ctx->tuning;
  vs_plan_layout(n_lanes, tab.costab_len, &sh, &b);

  const double t_host1 = vs_now_ms();
  hipError_t e = hipSetDevice(ctx->device);
  if (zero_copy) {
    /* one pinned, device-mapped host block: the CPU writes the records, the kernel reads them over PCIe (a few
     * hundred bytes per utterance, once), the error word is read back by the CPU -- no copy engine involved */
    void *dev = NULL;
    if (e == hipSuccess) e = hipHostMalloc(&p->zc_host, b.zc_bytes, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, p->zc_host, 0);
    if (e == hipSuccess) {
      char *hb = (char *)p->zc_host, *db = (char *)dev;
      memcpy(hb, dl, b.lanes_bytes);
      if (b.cos_bytes) memcpy(hb + b.zc_off_cos, tab.costab, b.cos_bytes);
      p->zc_err = (int *)(hb + b.zc_off_err);
      *p->zc_err = 0;
      if (b.wide_bytes) memcpy(hb + b.zc_off_wide, tab.awide, b.wide_bytes);
      p->d_lanes = (VsDevLane *)db;
      p->d_costab = (double *)(db + b.zc_off_cos);
      p->d_err = (int *)(db + b.zc_off_err);
      if (b.wide_bytes) p->d_awide = (double *)(db + b.zc_off_wide);
    }
  } else {
    if (e == hipSuccess) e = plan_block_get(ctx, b.lanes_bytes, (void **)&p->d_lanes, &p->cap_lanes);
    if (e == hipSuccess) e = plan_block_get(ctx, b.small_bytes, (void **)&p->d_small, &p->cap_small);
    if (e == hipSuccess) {
      p->d_costab = (double *)p->d_small;
      p->d_err = (int *)(p->d_small + b.small_off_err);
      if (b.gmap_bytes) p->d_group_map = (VsGroupSlot *)(p->d_small + b.small_off_gmap);
    }
    if (e == hipSuccess && b.wide_bytes) e = hipMalloc((void **)&p->d_awide, b.wide_bytes);
  }
  if (e == hipSuccess) p->d_taps = p->d_costab + tab.taps_off;
  if (e == hipSuccess && sh.wave_specialised) e = plan_block_get(ctx, (n_samples + 32) * sizeof(int16_t), (void **)&p->d_sink, &p->cap_sink);
  if (e == hipSuccess && b.gmap_bytes && zero_copy) e = hipMalloc((void **)&p->d_group_map, b.gmap_bytes);
  if (e == hipSuccess && sh.ondw_pitch)
    e = plan_block_get(ctx, n_lanes * (size_t)sh.ondw_pitch * sizeof(float), (void **)&p->d_ondw, &p->cap_ondw);
  if (e == hipSuccess && sh.pow_lframe) e = plan_block_get(ctx, n_lanes * sizeof(int32_t), (void **)&p->d_odone, &p->cap_odone);
  if (e == hipSuccess && sh.wide && !filter_only) {
    const size_t flow_bytes = n_lanes * sh.flow_pitch * sizeof(int16_t);
    if (mode & VS_PLAN_POOL_SCRATCH) {
      /* grows only with the first (largest) chunk of a pipeline, i.e. while nothing runs */
      if (vs_pool_device(ctx, &ctx->pool.d_flow, &ctx->pool.d_flow_bytes, flow_bytes) != VS_OK) e = hipErrorOutOfMemory;
      p->d_flow = (int16_t *)ctx->pool.d_flow;
      p->owns_flow = 0;
    } else {
      e = hipMalloc((void **)&p->d_flow, flow_bytes);
      p->owns_flow = 1;
    }
  }
  if (!zero_copy) {
    /* the records go up on a stream of the context's own -- inside a chunk pipeline on the pipeline's upload stream --,
     * never on the launch stream: the wait below is for THESE copies and not for whatever kernel the caller has running
     * (the previous chunk's, or batch k's while batch k + 1 is being planned); the launch that uses the records is
     * enqueued after this function has returned, i.e. after the copies have completed */
    hipStream_t up = ctx->upload;
    if (!up) {
      if (e == hipSuccess) e = vs_own_upload(ctx);
      up = ctx->own_upload;
    }
    if (e == hipSuccess && b.wide_bytes) e = hipMemcpyAsync(p->d_awide, tab.awide, b.wide_bytes, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = small_block_upload(ctx, p, &b, &tab, sh.gmap, up, &small_tmp);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_lanes, dl, b.lanes_bytes, hipMemcpyHostToDevice, up);
    if (e == hipSuccess) e = hipStreamSynchronize(up);
  }
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    vs_plan_destroy(p); /* frees whatever was allocated */
    rc = VS_ERR_HIP;
    goto done;
  }
  const double t_host2 = vs_now_ms();
  p->host_ms = t_host1 - t_host0;
  p->upload_ms = t_host2 - t_host1;
  *out = p;
done:
  vs_plan_tables_release(&tab);
  free(sh.gmap);
  free(small_tmp);
  return rc;
}

int vs_plan_create(vs_ctx *ctx, const vs_lane *lanes, size_t n_lanes, size_t n_samples,
                              vs_plan **out)
{
  return vs_plan_create_impl(ctx, lanes, n_lanes, n_samples, 0, out);
}

void vs_plan_destroy(vs_plan *p)
{
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  /* the blocks every plan has go back to the context's cache, behind the launches that still read them (no hipFree, which
   * would wait for the device: plan_block_put); the rare ones are freed */
  vs_ctx *ctx = p->ctx;
  VsRetire *retire = NULL;
  if (p->last_launch) {
    retire = (VsRetire *)malloc(sizeof(VsRetire));
    if (retire) {
      retire->ev = p->last_launch;
      retire->refs = 1; /* ours, until the blocks have theirs */
    } else { /* no memory for 16 bytes: wait here instead */
      (void)hipEventSynchronize(p->last_launch);
      (void)hipEventDestroy(p->last_launch);
    }
  }
  if (p->zc_host) {
    (void)hipHostFree(p->zc_host); /* records, cos rows, error word and wide taps of a zero-copy plan */
  } else {
    plan_block_put(ctx, p->d_lanes, p->cap_lanes, retire);
    plan_block_put(ctx, p->d_small, p->cap_small, retire); /* cos rows + taps, the mixed-rings table, the error word */
    if (p->d_awide) (void)hipFree(p->d_awide);
  }
  plan_block_put(ctx, p->d_sink, p->cap_sink, retire);
  if (p->d_seeds) (void)hipFree(p->d_seeds);
  if (p->h_seeds) (void)hipHostFree(p->h_seeds);
  if (p->seeds_copied) (void)hipEventDestroy(p->seeds_copied);
  if (p->d_group_map && !p->d_small) (void)hipFree(p->d_group_map); /* (inside d_small when the plan copies) */
  plan_block_put(ctx, p->d_ondw, p->cap_ondw, retire);
  plan_block_put(ctx, p->d_odone, p->cap_odone, retire);
  if (p->d_flow && p->owns_flow) (void)hipFree(p->d_flow);
  retire_unref(retire);
  free(p);
}

/* behind every launch of a plan: the event its device blocks will retire behind (plan_block_put) */
static int plan_mark_launch(vs_plan *p)
{
  vs_ctx *ctx = p->ctx;
  if (!p->last_launch) VS_HIP(ctx, hipEventCreateWithFlags(&p->last_launch, hipEventDisableTiming));
  /* a caller who moved the context to another stream between two launches of this plan: the new stream waits for the old
   * launches first, so that the event recorded on it still stands behind EVERY launch that reads the plan's blocks */
  else if (p->last_stream != ctx->stream) VS_HIP(ctx, hipStreamWaitEvent(ctx->stream, p->last_launch, 0));
  VS_HIP(ctx, hipEventRecord(p->last_launch, ctx->stream));
  p->last_stream = ctx->stream;
  return VS_OK;
}

int vs_plan_status(vs_plan *p, int *flags)
{
  if (!p) return VS_ERR_ARG;
  vs_ctx *ctx = p->ctx;
  int word = 0;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  if (p->zc_err) { /* zero-copy plan: the word lives in host memory the device writes through PCIe */
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    word = *(volatile int *)p->zc_err;
  } else {
    VS_HIP(ctx, hipMemcpyAsync(&word, p->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (flags) *flags = word;
  return word ? VS_ERR_INTERNAL : VS_OK;
}

int vs_plan_reseed(vs_plan *p, const uint64_t *seeds, const uint64_t *out_seeds)
{
  if (!p || !seeds) return VS_ERR_ARG;
  if (p->filter_only && !out_seeds) out_seeds = seeds;
  if (!out_seeds) out_seeds = seeds;
  vs_ctx *ctx = p->ctx;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = p->n_lanes;
  if (p->zc_host) return VS_ERR_INTERNAL; /* (the small calls' zero-copy plans live for one call inside vs_source / vs_filter) */
  if (!p->seeds_copied) {
    /* all three or none: a first call that fails half-way leaves the plan as it was, and the next one starts over */
    unsigned long long *d = NULL, *h = NULL;
    hipEvent_t ev = NULL;
    hipError_t e = hipMalloc((void **)&d, 2 * n * sizeof(uint64_t));
    if (e == hipSuccess) e = hipHostMalloc((void **)&h, 2 * n * sizeof(uint64_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) {
      if (d) (void)hipFree(d);
      if (h) (void)hipHostFree(h);
      ctx->last_hip_error = (int)e;
      return e == hipErrorOutOfMemory ? VS_ERR_NOMEM : VS_ERR_HIP;
    }
    p->d_seeds = d;
    p->h_seeds = h;
    p->seeds_copied = ev;
  } else {
    VS_HIP(ctx, hipEventSynchronize(p->seeds_copied)); /* the previous reseed's upload has left the pinned buffer */
  }
  /* the caller's arrays are his again when this returns: they go through the plan's pinned buffer */
  memcpy(p->h_seeds, seeds, n * sizeof(uint64_t));
  memcpy(p->h_seeds + n, out_seeds, n * sizeof(uint64_t));
  /* on the launch stream: behind the launches that still read the old seeds, in front of the next one */
  VS_HIP(ctx, hipMemcpyAsync(p->d_seeds, p->h_seeds, 2 * n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  VS_HIP(ctx, hipEventRecord(p->seeds_copied, ctx->stream));
  VS_HIP(ctx, vs_launch_reseed(p->d_lanes, p->d_seeds, p->d_seeds + n, (int)n, ctx->stream));
  return plan_mark_launch(p); /* (the reseed kernel writes the records: the blocks retire behind it) */
}

/* diagnostic builds (tools/diag_bench.py): device buffer of grid*8 uint64 cycle counters */
int vs_plan_set_diag(vs_plan *p, void *diag_dev)
{
  if (!p) return VS_ERR_ARG;
  p->d_diag = (unsigned long long *)diag_dev;
  return VS_OK;
}

int vs_plan_timing(const vs_plan *p, double *host_ms, double *upload_ms)
{
  if (!p) return VS_ERR_ARG;
  if (host_ms) *host_ms = p->host_ms;
  if (upload_ms) *upload_ms = p->upload_ms;
  return VS_OK;
}

/* the fields of a launch's arguments that say which kernel runs and in what geometry: the plan's shape and which of its
 * tables the kind uses (vs_plan_launch fills in the rest) */
static void plan_pick_args(const vs_plan *p, int kind, VsKernelArgs *a)
{
  const VsPlanShape *s = &p->shape;
  a->n_lanes = (int)p->n_lanes;
  a->n_samples = (int)p->n_samples;
  a->ondw = (kind == VS_KIND_SOURCE) ? NULL : p->d_ondw;
  a->ondw_pitch = s->ondw_pitch;
  a->ws_pairs = s->ws_pairs;
  a->ws_roles = s->ws_roles;
  a->ws_layout = s->ws_layout;
  a->group_map = p->d_group_map;
  a->group_lanes = s->group_lanes;
  a->ws_pair_bytes = s->ws_pair_bytes;
}
/* what a step adds to the arguments of its launch and of those behind it */
static void plan_step_args(const vs_plan *p, const VsLaunchStep *st, VsKernelArgs *a)
{
  if (st->awide) a->awide = p->d_awide;
  if (st->pow) {
    a->odone = p->d_odone;
    a->pow_lframe = p->shape.pow_lframe;
  }
  if (st->from_flow) {
    a->in = p->d_flow;
    a->in_pitch = (long)p->shape.flow_pitch;
    a->log = NULL;
    a->ncyc = NULL;
  }
}

/* The kernels of a launch without a cycle log: its steps, each through the selection its launcher asks.  (As ever, a wide
 * plan's name ends with the wide filter kernel, and its source kernel goes without the narrow build's remark.) */
int vs_plan_kernel_name(const vs_plan *p, int kind, char *buf, size_t len)
{
  if (!p || !buf || len == 0) return VS_ERR_ARG;
  const VsPlanShape *s = &p->shape;
  VsKernelArgs a;
  memset(&a, 0, sizeof(a));
  plan_pick_args(p, kind, &a);
  VsLaunchStep steps[VS_PLAN_MAX_STEPS];
  const int n = vs_plan_steps(s, p->ctx->arith, kind, false, a.ondw != NULL, steps);
  char name[256] = "", one[64];
  for (int k = 0; k < n; k++) {
    const VsLaunchStep *st = &steps[k];
    VsLaunchPick pick = {0};
    VsOutNoisePick passes;
    memset(&passes, 0, sizeof(passes));
    plan_step_args(p, st, &a);
    /* (a launch the launcher would refuse still has its kernel named) */
    if (st->what == VS_STEP_KERNEL)
      (void)vs_launch_pick(st->arith, st->kind, st->log, st->wave_specialised, st->pre1, &a, s->grid, st->lds_bytes, &pick);
    else if (st->what == VS_STEP_FILTER_WIDE) (void)vs_launch_pick_wide(st->arith, &a, s->grid, &pick);
    else (void)vs_launch_pick_out_noise(&a, 1, 1, &passes);
    const int ids[2] = {st->what == VS_STEP_OUT_NOISE ? passes.power.kernel : pick.kernel, passes.noise.kernel};
    for (int i = 0; i < 2 && ids[i]; i++) {
      const size_t used = strlen(name);
      vs_kernel_id_name(ids[i], one, sizeof(one));
      snprintf(name + used, sizeof(name) - used, "%s%s%s", used ? " + " : "", one,
               (VS_KERNEL_FAMILY(ids[i]) == VS_KF_NARROW && !st->into_flow) ? " (narrow build: 16 utterances per wavefront)" : "");
    }
    if (st->what == VS_STEP_FILTER_WIDE) break;
  }
  snprintf(buf, len, "%s", name);
  return VS_OK;
}

int vs_plan_roles(const vs_plan *p, int *roles, int *layout, int *simd_fallback)
{
  if (!p) return VS_ERR_ARG;
  if (roles) *roles = p->shape.wave_specialised ? p->shape.ws_roles : 1;
  if (layout) *layout = p->shape.wave_specialised ? p->shape.ws_layout : 0;
  if (simd_fallback) *simd_fallback = p->shape.simd_fallback;
  return VS_OK;
}

int vs_plan_info(const vs_plan *p, size_t *lds_bytes, size_t *n_workgroups,
                            size_t *ring_slots)
{
  if (!p) return VS_ERR_ARG;
  if (lds_bytes) *lds_bytes = p->shape.lds_bytes;
  if (n_workgroups) *n_workgroups = p->shape.grid;
  if (ring_slots) *ring_slots = (size_t)p->shape.ring_slots;
  return VS_OK;
}

int vs_plan_launch(vs_plan *p, int kind, const int16_t *in_dev, size_t in_pitch,
                              int16_t *out_dev, size_t out_pitch, vs_cycle_rec *log_dev,
                              size_t log_pitch, int32_t *ncyc_dev)
{
  if (!p || !out_dev) return VS_ERR_ARG;
  if (kind != VS_KIND_SYNTH && kind != VS_KIND_SOURCE && kind != VS_KIND_FILTER) return VS_ERR_ARG;
  if (out_pitch < p->n_samples) return VS_ERR_ARG;
  if (kind == VS_KIND_FILTER && (!in_dev || in_pitch < p->n_samples)) return VS_ERR_ARG;
  if (p->filter_only && kind != VS_KIND_FILTER) return VS_ERR_ARG;
  if (log_dev && log_pitch == 0) return VS_ERR_ARG;
  vs_ctx *ctx = p->ctx;
  const VsPlanShape *s = &p->shape;
  VsLaunchKnobs k;
  vs_plan_knobs(s, &p->tuning, ctx->arith, &k);
  VsKernelArgs a;
  memset(&a, 0, sizeof(a));
  a.lanes = p->d_lanes;
  a.costab = p->d_costab;
  a.taps = p->d_taps;
  a.in = in_dev;
  a.out = out_dev;
  a.log = (kind == VS_KIND_FILTER) ? NULL : (void *)log_dev;
  a.ncyc = ncyc_dev;
  a.in_pitch = (long)in_pitch;
  a.out_pitch = (long)out_pitch;
  a.log_pitch = (long)log_pitch;
  plan_pick_args(p, kind, &a);
  a.ring_slots = s->ring_slots;
  a.ltab_entries = s->ltab_entries;
  a.ready_min = k.ready_min;
  a.diag = p->d_diag;
  a.err = p->d_err;
  a.sink = p->d_sink;
  a.gen_min = k.gen_min;
  a.gen_low = k.gen_low;
  a.spin_limit = k.spin_limit;
  a.fault = p->tuning.fault;
  a.ws_filter_prio = k.ws_filter_prio;
  /* 16-byte vector stores need every row start 4-byte aligned */
  int vec = ((out_pitch & 1) == 0) && ((((uintptr_t)out_dev) & 3) == 0);
  if (kind == VS_KIND_FILTER) vec = vec && ((in_pitch & 1) == 0) && ((((uintptr_t)in_dev) & 3) == 0);
  a.vec_ok = vec;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VsLaunchStep steps[VS_PLAN_MAX_STEPS];
  const int n_steps = vs_plan_steps(s, ctx->arith, kind, a.log != NULL, a.ondw != NULL, steps);
  for (int i = 0; i < n_steps; i++) {
    const VsLaunchStep *st = &steps[i];
    plan_step_args(p, st, &a);
    VsKernelArgs now = a;
    if (st->into_flow) {
      now.out = p->d_flow;
      now.out_pitch = (long)s->flow_pitch;
      now.ondw = NULL;
      now.vec_ok = 1; /* rows of the plan's own buffer start 16-byte aligned */
    }
    hipError_t e;
    if (st->what == VS_STEP_KERNEL)
      e = vs_launch_kernel(st->arith, st->kind, st->log, st->wave_specialised, st->pre1, &now, s->grid, st->lds_bytes, ctx->stream);
    else if (st->what == VS_STEP_FILTER_WIDE) e = vs_launch_filter_wide(st->arith, &now, s->grid, ctx->stream);
    else e = vs_launch_out_noise(&now, ctx->stream);
    VS_HIP(ctx, e);
  }
  return plan_mark_launch(p);
}

