/*
 * vs_blocks.c -- the device blocks a context keeps between calls, the one path on which the per-row records of a launch
 * (vs_measure_launch, vs_lpc_launch, vs_iaif_launch, vs_cplpc_launch, vs_track_launch, vs_inverse_launch) reach the device, and the one
 * path on which the host-buffer calls over those launches move the caller's arrays:
 *   the cache of retired blocks (plan_block_get / plan_block_put): plans and record uploads take their blocks from it;
 *   the record upload (vs_rec_stage / vs_rec_upload / vs_rec_retire): a pinned block per feature, the copy on own_upload,
 *   the device block back into the cache behind the kernel that read it; the same with a scratch block next to the
 *   records (vs_rec_upload_scratch / vs_rec_retire_both) for vs_guided_launch, vs_psola_launch and vs_psola_ts_launch;
 *   the pool's device buffers (vs_pool_device) and the host-buffer call on them (vs_host_begin / vs_host_end).
 * Plain C against the HIP runtime's C API; tests/c/test_blocks_asan.c and tests/c/test_hostcall_asan.c run it against a
 * stand-in runtime.
 */
#include <stdlib.h>

#include "vs_internal.h"

void retire_unref(VsRetire *r)
{
  if (r && --r->refs == 0) {
    (void)hipEventDestroy(r->ev);
    free(r);
  }
}
/* A device block of at least `bytes` for a plan: a retired one of a fitting size (at most twice what is asked for -- a
 * plan of 64 utterances does not sit on the 8 MB of a batch's records) once the launches that read it are over, or a new
 * one.  *cap = what it really holds. */
hipError_t plan_block_get(vs_ctx *ctx, size_t bytes, void **ptr, size_t *cap)
{
  if (bytes == 0) bytes = 1;
  /* of the fitting blocks the one that has been retired longest: its launches are most likely over already (the block of
   * the plan destroyed a moment ago would make this call wait for a kernel that has only just started) */
  int best = -1;
  for (int k = 0; k < VS_PLAN_CACHE_SLOTS; k++) {
    const VsBlock *b = &ctx->plan_cache[k];
    if (b->ptr && b->bytes >= bytes && b->bytes <= 2 * bytes + 4096 && (best < 0 || b->stamp < ctx->plan_cache[best].stamp)) best = k;
  }
  if (best >= 0) {
    VsBlock *b = &ctx->plan_cache[best];
    hipError_t e = b->retired ? hipEventSynchronize(b->retired->ev) : hipSuccess;
    retire_unref(b->retired);
    *ptr = b->ptr;
    *cap = b->bytes;
    b->ptr = NULL;
    b->retired = NULL;
    if (e == hipSuccess) return hipSuccess;
    (void)hipFree(*ptr); /* cannot tell whether it is still read: not ours to hand on */
    (void)hipGetLastError();
  }
  *cap = bytes;
  return hipMalloc(ptr, bytes);
}
/* ... and back, when its plan is destroyed: behind the plan's last launch (retire: shared by the plan's blocks, NULL if it
 * was never launched).  A full cache gives up its oldest block (hipFree: that one wait for the device is the price of the
 * 33rd retired block). */
void plan_block_put(vs_ctx *ctx, void *ptr, size_t cap, VsRetire *retire)
{
  if (!ptr) return;
  int slot = -1, oldest = 0;
  for (int k = 0; k < VS_PLAN_CACHE_SLOTS; k++) {
    if (!ctx->plan_cache[k].ptr) {
      slot = k;
      break;
    }
    if (ctx->plan_cache[k].stamp < ctx->plan_cache[oldest].stamp) oldest = k;
  }
  if (slot < 0) {
    VsBlock *b = &ctx->plan_cache[oldest];
    retire_unref(b->retired);
    (void)hipFree(b->ptr);
    b->ptr = NULL;
    slot = oldest;
  }
  VsBlock *b = &ctx->plan_cache[slot];
  if (cap == 0) {
    (void)hipFree(ptr);
    return;
  }
  b->ptr = ptr;
  b->bytes = cap;
  b->retired = retire;
  if (retire) retire->refs++;
  b->stamp = ++ctx->plan_cache_stamp;
}
void vs_plan_cache_release(vs_ctx *ctx)
{
  (void)hipSetDevice(ctx->device);
  for (int k = 0; k < VS_PLAN_CACHE_SLOTS; k++) {
    VsBlock *b = &ctx->plan_cache[k];
    if (!b->ptr) continue;
    retire_unref(b->retired);
    (void)hipFree(b->ptr);
    b->ptr = NULL;
    b->retired = NULL;
  }
}

/* The context's own upload stream, made on first use: NON-BLOCKING, never the legacy stream -- that one waits for every
 * blocking stream of the process, the caller's running kernel included, and what goes up here goes up next to a launch */
hipError_t vs_own_upload(vs_ctx *ctx)
{
  return ctx->own_upload ? hipSuccess : hipStreamCreateWithFlags(&ctx->own_upload, hipStreamNonBlocking);
}

/* ---- the record upload: stage, fill *host, upload, launch, retire ---- */

int vs_rec_stage(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, void **host)
{
  VS_HIP(ctx, hipSetDevice(ctx->device));
  VS_HIP(ctx, vs_own_upload(ctx));
  if (!slot->copied) VS_HIP(ctx, hipEventCreateWithFlags(&slot->copied, hipEventDisableTiming));
  /* the pinned block is free once the previous upload out of it has run (own_upload: nothing else queues there long) */
  VS_HIP(ctx, hipEventSynchronize(slot->copied));
  if (slot->pin_bytes < bytes) {
    if (slot->pin) (void)hipHostFree(slot->pin);
    slot->pin = NULL;
    slot->pin_bytes = 0;
    VS_HIP(ctx, hipHostMalloc(&slot->pin, bytes, hipHostMallocDefault));
    slot->pin_bytes = bytes;
  }
  *host = slot->pin;
  return VS_OK;
}

int vs_rec_upload(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk)
{
  VS_HIP(ctx, plan_block_get(ctx, bytes, &blk->dev, &blk->cap));
  hipError_t e = hipMemcpyAsync(blk->dev, slot->pin, bytes, hipMemcpyHostToDevice, ctx->own_upload);
  if (e == hipSuccess) e = hipEventRecord(slot->copied, ctx->own_upload);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, slot->copied, 0);
  return e == hipSuccess ? VS_OK : vs_rec_retire(ctx, blk, e);
}

int vs_rec_retire(vs_ctx *ctx, VsRecBlock *blk, hipError_t launched)
{
  /* the block goes back to the context's cache behind the kernels that read it (no hipFree: it would wait for the
   * device) */
  hipError_t e = launched;
  hipEvent_t done = NULL;
  if (e == hipSuccess) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventRecord(done, ctx->stream);
  VsRetire *retire = NULL;
  if (e == hipSuccess && (retire = (VsRetire *)malloc(sizeof(VsRetire))) != NULL) {
    retire->ev = done;
    retire->refs = 1;
    plan_block_put(ctx, blk->dev, blk->cap, retire);
    retire_unref(retire);
  } else {
    if (done) {
      (void)hipEventSynchronize(done);
      (void)hipEventDestroy(done);
    } else {
      (void)hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(blk->dev);
  }
  blk->dev = NULL;
  if (e != hipSuccess) {
    ctx->last_hip_error = (int)e;
    return VS_ERR_HIP;
  }
  return retire ? VS_OK : VS_ERR_NOMEM;
}

/* ---- ... and a launch whose kernels also need scratch: a second block of the cache, got before the records go up ---- */

int vs_rec_upload_scratch(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk, size_t scratch_bytes,
                          VsRecBlock *scratch)
{
  scratch->dev = NULL;
  scratch->cap = 0;
  VS_HIP(ctx, plan_block_get(ctx, scratch_bytes, &scratch->dev, &scratch->cap));
  const int rc = vs_rec_upload(ctx, slot, bytes, blk);
  if (rc != VS_OK) {
    plan_block_put(ctx, scratch->dev, scratch->cap, NULL); /* nothing was enqueued that reads it */
    scratch->dev = NULL;
  }
  return rc;
}

int vs_rec_retire_both(vs_ctx *ctx, VsRecBlock *blk, VsRecBlock *scratch, hipError_t launched)
{
  const int rc = vs_rec_retire(ctx, blk, launched);
  const int rc2 = vs_rec_retire(ctx, scratch, launched);
  return rc != VS_OK ? rc : rc2;
}

void vs_rec_release(vs_ctx *ctx, VsRecSlot *slot)
{
  (void)hipSetDevice(ctx->device);
  if (slot->copied) {
    (void)hipEventSynchronize(slot->copied);
    (void)hipEventDestroy(slot->copied);
    slot->copied = NULL;
  }
  if (slot->pin) (void)hipHostFree(slot->pin);
  slot->pin = NULL;
  slot->pin_bytes = 0;
}

/* ---- the pool's device buffers, and the host-buffer call: begin, the feature's launch, end ---- */

int vs_pool_device(vs_ctx *ctx, void **ptr, size_t *have, size_t bytes)
{
  if (*ptr && *have >= bytes) return VS_OK;
  VS_HIP(ctx, hipSetDevice(ctx->device));
  if (*ptr) {
    void *old = *ptr; /* given up whatever hipFree answers: a buffer that may be gone is not kept */
    *ptr = NULL;
    *have = 0;
    VS_HIP(ctx, hipFree(old)); /* waits for the device: only between pipelines */
  }
  const size_t want = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  VS_HIP(ctx, hipMalloc(ptr, want));
  *have = want;
  return VS_OK;
}

static int part_present(const VsHostPart *p) { return p->host && p->bytes; }
static size_t part_room(const VsHostPart *p) { return (p->bytes + 255) & ~(size_t)255; }

int vs_host_begin(vs_ctx *ctx, const void *in, size_t in_bytes, VsHostPart *parts, int n_parts)
{
  VS_HIP(ctx, hipSetDevice(ctx->device));
  /* every part starts 256-byte aligned and d_aux holds the sum of the rounded sizes: the layout is nobody else's */
  size_t total = 0;
  for (int k = 0; k < n_parts; k++) {
    parts[k].dev = NULL;
    if (part_present(&parts[k])) total += part_room(&parts[k]);
  }
  int rc = vs_pool_device(ctx, &ctx->pool.d_in, &ctx->pool.d_in_bytes, in_bytes);
  if (rc == VS_OK) rc = vs_pool_device(ctx, &ctx->pool.d_aux, &ctx->pool.d_aux_bytes, total);
  if (rc != VS_OK) return rc;
  VS_HIP(ctx, hipMemcpyAsync(ctx->pool.d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  char *next = (char *)ctx->pool.d_aux;
  for (int k = 0; k < n_parts; k++) {
    VsHostPart *p = &parts[k];
    if (!part_present(p)) continue;
    p->dev = next;
    next += part_room(p);
    if (p->flags & VS_PART_FILL_FF) VS_HIP(ctx, hipMemsetAsync(p->dev, 0xFF, p->bytes, ctx->stream));
    else if (p->flags & VS_PART_UP) VS_HIP(ctx, hipMemcpyAsync(p->dev, p->host, p->bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  return VS_OK;
}

int vs_host_end(vs_ctx *ctx, int launch_rc, const VsHostPart *parts, int n_parts)
{
  if (launch_rc != VS_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return launch_rc;
  }
  for (int k = 0; k < n_parts; k++) {
    const VsHostPart *p = &parts[k];
    if (p->dev && (p->flags & VS_PART_DOWN))
      VS_HIP(ctx, hipMemcpyAsync(p->host, p->dev, p->bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  VS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VS_OK;
}
