/* The block cache and the record upload (csrc/vs_blocks.c) against the stand-in HIP runtime of hip_standin.h, which
 * counts the calls it gets and can fail the k-th one; the module's own malloc (the VsRetire of a launch) goes through a
 * counter of its own.
 * Checked: what a slot and the cache hold over three rounds of different sizes; for every call of a round -- on a fresh
 * context and on a used one -- that failing it gives the return the library documents, leaves the context usable and
 * leaks nothing; a failed launch; the same for the launches that take a scratch block next to their records.
 * Host logic only, under ASan/UBSan with leak detection (tests/test_host_sanitizers.py). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the module's malloc: fails when the countdown reaches zero */
static int malloc_fail_in;
static void *test_malloc(size_t n)
{
  if (malloc_fail_in > 0 && --malloc_fail_in == 0) return NULL;
  return malloc(n);
}
#define malloc test_malloc
#include "../../voice_synth_amd/csrc/vs_blocks.c"
#undef malloc

#include "hip_standin.h"

/* ---- one launch the way the three host files make it: stage, fill, upload, launch, retire ---- */
static int one_round(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, hipError_t launched, void **dev)
{
  void *host = NULL;
  VsRecBlock blk;
  int rc = vs_rec_stage(ctx, slot, bytes, &host);
  if (rc != VS_OK) return rc;
  CHECK(host == slot->pin && slot->pin_bytes >= bytes);
  memset(host, (int)(bytes & 0xFF), bytes);
  rc = vs_rec_upload(ctx, slot, bytes, &blk);
  if (rc != VS_OK) return rc;
  CHECK(blk.cap >= bytes && memcmp(blk.dev, host, bytes) == 0);
  if (dev) *dev = blk.dev;
  return vs_rec_retire(ctx, &blk, launched);
}

static void release(vs_ctx *ctx)
{
  VsRecSlot *slots[3] = {&ctx->rec_measure, &ctx->rec_lpc, &ctx->rec_track};
  for (int k = 0; k < 3; k++) {
    vs_rec_release(ctx, slots[k]);
    CHECK(!slots[k]->pin && !slots[k]->pin_bytes && !slots[k]->copied);
  }
  vs_plan_cache_release(ctx);
  if (ctx->own_upload) (void)hipStreamDestroy(ctx->own_upload);
  CHECK(dev_live == 0 && pin_live == 0 && ev_live == 0 && stream_live == 0);
  free(ctx);
}

static vs_ctx *new_ctx(void)
{
  vs_ctx *ctx = (vs_ctx *)calloc(1, sizeof(vs_ctx));
  if (!ctx) exit(2);
  calls = fail_at = 0;
  return ctx;
}

static void happy_path(void)
{
  vs_ctx *ctx = new_ctx();
  VsRecSlot *slot = &ctx->rec_lpc;
  void *dev1 = NULL, *dev2 = NULL, *dev3 = NULL;
  CHECK(one_round(ctx, slot, 1000, hipSuccess, &dev1) == VS_OK);
  CHECK(pin_allocs == 1 && pin_frees == 0 && dev_allocs == 1 && slot->pin_bytes == 1000);
  /* larger: another pinned block, the first one freed; another device block, the first one stays in the cache */
  CHECK(one_round(ctx, slot, 5000, hipSuccess, &dev2) == VS_OK);
  CHECK(pin_allocs == 2 && pin_frees == 1 && pin_live == 1 && slot->pin_bytes == 5000);
  CHECK(dev_allocs == 2 && dev_live == 2 && dev2 != dev1);
  /* small enough for the first round's device block (both fit; the one retired longest is taken); the pinned block stays */
  CHECK(one_round(ctx, slot, 600, hipSuccess, &dev3) == VS_OK);
  CHECK(dev3 == dev1 && dev_allocs == 2 && dev_live == 2 && pin_allocs == 2 && slot->pin_bytes == 5000);
  CHECK(ev_live == 3 && stream_syncs == 0 && ctx->last_hip_error == 0); /* the slot's event, one per cached block */
  /* the other slots are not touched */
  CHECK(!ctx->rec_measure.copied && !ctx->rec_track.copied);
  release(ctx);
}

/* Every call of one round fails in turn.  used = 0: the round is the context's first (own_upload, the slot's event, both
 * blocks are made in it); used = 1: a smaller round of the slot came before, so this one grows the pinned block, and
 * a round of its size on another slot, so this one takes its device block from the cache. */
static void injection_sweep(int used)
{
  int n_calls = 0;
  for (int k = 0; n_calls == 0 || k <= n_calls; k++) { /* k = 0: the clean run that counts the calls */
    vs_ctx *ctx = new_ctx();
    VsRecSlot *slot = &ctx->rec_track;
    if (used) {
      CHECK(one_round(ctx, &ctx->rec_lpc, 3000, hipSuccess, NULL) == VS_OK);
      CHECK(one_round(ctx, slot, 100, hipSuccess, NULL) == VS_OK);
      CHECK(dev_live == 1 && slot->pin_bytes == 100);
    }
    const int dev_before = dev_live;
    calls = 0;
    fail_at = k;
    failed_fn = NULL;
    ctx->last_hip_error = 0;
    const int rc = one_round(ctx, slot, 3000, hipSuccess, NULL);
    fail_at = 0;
    if (k == 0) {
      CHECK(rc == VS_OK && calls == 11); /* both kinds of round happen to make eleven calls */
      n_calls = calls;
    } else {
      CHECK(failed_fn != NULL);
      /* nothing to be done about a call that gives something back; an event of the cache that cannot be waited for
       * costs its block, and a new one is made; every other failure is the call's */
      const int ignored = !strcmp(failed_fn, "hipFree") || !strcmp(failed_fn, "hipHostFree") ||
                          !strcmp(failed_fn, "hipEventDestroy") ||
                          (!strcmp(failed_fn, "hipEventSynchronize") && failed_ev != (void *)slot->copied);
      CHECK(!ignored || used);
      CHECK(rc == (ignored ? VS_OK : VS_ERR_HIP));
      CHECK(ctx->last_hip_error == (ignored ? 0 : (int)hipErrorUnknown));
      if (rc != VS_OK) CHECK(dev_live <= dev_before); /* the block of the failed round is not kept */
    }
    CHECK(one_round(ctx, slot, 3000, hipSuccess, NULL) == VS_OK);
    release(ctx);
  }
}

/* ---- a launch that also takes scratch, the way vs_guided_launch and the two PSOLA launches make it ---- */
static int calls_at_upload; /* the runtime calls made when the last round reached vs_rec_upload_scratch (-1: it did not) */
static int scratch_round(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, size_t scratch_bytes, hipError_t launched)
{
  void *host = NULL;
  VsRecBlock blk, scratch;
  calls_at_upload = -1;
  int rc = vs_rec_stage(ctx, slot, bytes, &host);
  if (rc != VS_OK) return rc;
  memset(host, (int)(bytes & 0xFF), bytes);
  calls_at_upload = calls;
  rc = vs_rec_upload_scratch(ctx, slot, bytes, &blk, scratch_bytes, &scratch);
  if (rc != VS_OK) return rc;
  CHECK(blk.cap >= bytes && memcmp(blk.dev, host, bytes) == 0 && scratch.dev != blk.dev && scratch.cap >= scratch_bytes);
  memset(scratch.dev, 0x5A, scratch_bytes); /* the kernels' scratch, to the last byte */
  rc = vs_rec_retire_both(ctx, &blk, &scratch, launched);
  CHECK(!blk.dev && !scratch.dev);
  return rc;
}

/* the cache's blocks that no event guards */
static int unretired(const vs_ctx *ctx)
{
  int n = 0;
  for (int k = 0; k < VS_PLAN_CACHE_SLOTS; k++) n += ctx->plan_cache[k].ptr && !ctx->plan_cache[k].retired;
  return n;
}

/* Every call of such a round fails in turn: the scratch block's get, the record block's get, the copy, the event
 * record, the stream wait, the retire events.  used = 0: the context's first round, both blocks are new; used = 1: both
 * come out of the cache, and the pinned block grows.  A round whose upload fails behind the scratch's get leaves the
 * scratch in the cache with no retire event -- nothing was enqueued that reads it --, and the next round takes it. */
static void scratch_sweep(int used)
{
  int n_calls = 0;
  for (int k = 0; n_calls == 0 || k <= n_calls; k++) {
    vs_ctx *ctx = new_ctx();
    VsRecSlot *slot = &ctx->rec_track;
    if (used) {
      CHECK(one_round(ctx, &ctx->rec_lpc, 3000, hipSuccess, NULL) == VS_OK);
      CHECK(one_round(ctx, &ctx->rec_lpc, 7000, hipSuccess, NULL) == VS_OK);
      CHECK(one_round(ctx, slot, 100, hipSuccess, NULL) == VS_OK);
      CHECK(dev_live == 2 && slot->pin_bytes == 100 && unretired(ctx) == 0);
    }
    const int dev_before = dev_live;
    calls = 0;
    fail_at = k;
    failed_fn = NULL;
    ctx->last_hip_error = 0;
    const int rc = scratch_round(ctx, slot, 3000, 7000, hipSuccess);
    fail_at = 0;
    if (k == 0) {
      /* stage; a block for the scratch; a block, the copy, the event and the wait for the records; two retires */
      CHECK(rc == VS_OK && calls == (used ? 15 : 14) && dev_live == 2 && unretired(ctx) == 0);
      n_calls = calls;
    } else {
      CHECK(failed_fn != NULL);
      const int ignored = !strcmp(failed_fn, "hipFree") || !strcmp(failed_fn, "hipHostFree") ||
                          !strcmp(failed_fn, "hipEventDestroy") ||
                          (!strcmp(failed_fn, "hipEventSynchronize") && failed_ev != (void *)slot->copied);
      CHECK(!ignored || used);
      CHECK(rc == (ignored ? VS_OK : VS_ERR_HIP));
      CHECK(ctx->last_hip_error == (ignored ? 0 : (int)hipErrorUnknown));
      if (rc != VS_OK) CHECK(dev_live <= dev_before + 1); /* of a failed round at most the scratch is kept */
      /* the upload failed behind the scratch's get (on a fresh context that get is the first call): the scratch is back */
      const int in_upload = rc != VS_OK && calls_at_upload >= 0 && strcmp(failed_fn, "hipEventCreateWithFlags") != 0 &&
                            !(failed_ev && failed_ev != (void *)slot->copied);
      const int had_scratch = in_upload && (used || k > calls_at_upload + 1);
      CHECK(unretired(ctx) == had_scratch);
      /* the scratch kept; the records' block, if there was one, freed (used: that was one of the cache's two) */
      if (had_scratch) CHECK(dev_live == (used ? dev_before - 1 : dev_before + 1));
    }
    CHECK(scratch_round(ctx, slot, 3000, 7000, hipSuccess) == VS_OK && unretired(ctx) == 0);
    release(ctx);
  }
}

static void scratch_launch_fails(void)
{
  vs_ctx *ctx = new_ctx();
  const int syncs = stream_syncs;
  CHECK(scratch_round(ctx, &ctx->rec_measure, 3000, 7000, hipErrorLaunchFailure) == VS_ERR_HIP);
  CHECK(ctx->last_hip_error == (int)hipErrorLaunchFailure);
  CHECK(dev_live == 0 && ev_live == 1 && stream_syncs == syncs + 2); /* the stream waited for, then each block freed */
  malloc_fail_in = 2; /* the scratch's VsRetire: the records' block is cached, the scratch freed */
  CHECK(scratch_round(ctx, &ctx->rec_measure, 3000, 7000, hipSuccess) == VS_ERR_NOMEM);
  CHECK(malloc_fail_in == 0 && dev_live == 1);
  CHECK(scratch_round(ctx, &ctx->rec_measure, 3000, 7000, hipSuccess) == VS_OK);
  release(ctx);
}

static void retire_allocation_fails(void)
{
  vs_ctx *ctx = new_ctx();
  VsRecSlot *slot = &ctx->rec_measure;
  malloc_fail_in = 1;
  CHECK(one_round(ctx, slot, 3000, hipSuccess, NULL) == VS_ERR_NOMEM);
  CHECK(malloc_fail_in == 0 && ctx->last_hip_error == 0);
  CHECK(dev_live == 0 && ev_live == 1); /* the block freed behind the kernel's event, that event destroyed */
  CHECK(one_round(ctx, slot, 3000, hipSuccess, NULL) == VS_OK);
  release(ctx);
}

static void launch_fails(void)
{
  vs_ctx *ctx = new_ctx();
  VsRecSlot *slot = &ctx->rec_measure;
  const int syncs = stream_syncs;
  CHECK(one_round(ctx, slot, 3000, hipErrorLaunchFailure, NULL) == VS_ERR_HIP);
  CHECK(ctx->last_hip_error == (int)hipErrorLaunchFailure);
  CHECK(dev_live == 0 && ev_live == 1 && stream_syncs == syncs + 1); /* the stream waited for, then the block freed */
  CHECK(one_round(ctx, slot, 3000, hipSuccess, NULL) == VS_OK);
  release(ctx);
}

int main(void)
{
  happy_path();
  injection_sweep(0);
  injection_sweep(1);
  retire_allocation_fails();
  launch_fails();
  scratch_sweep(0);
  scratch_sweep(1);
  scratch_launch_fails();
  printf("ok\n");
  return 0;
}
