/* The "records + scratch" pair of csrc/vs_blocks.c for the host programs that bring their own stand-ins for the block
 * cache and the record upload (test_guided_host_asan.c, test_psola_host_asan.c, test_psola_ts_host_asan.c): the same
 * sequence over those stand-ins, so that blocks_out counts both blocks.  The real pair runs against a failing runtime in
 * test_blocks_asan.c.  Included behind the program's plan_block_get, plan_block_put, vs_rec_upload and vs_rec_retire. */
#ifndef REC_SCRATCH_STANDIN_H
#define REC_SCRATCH_STANDIN_H

int vs_rec_upload_scratch(vs_ctx *ctx, VsRecSlot *slot, size_t bytes, VsRecBlock *blk, size_t scratch_bytes,
                          VsRecBlock *scratch)
{
  scratch->dev = NULL;
  scratch->cap = 0;
  if (plan_block_get(ctx, scratch_bytes, &scratch->dev, &scratch->cap) != hipSuccess) return VS_ERR_HIP;
  const int rc = vs_rec_upload(ctx, slot, bytes, blk);
  if (rc != VS_OK) plan_block_put(ctx, scratch->dev, scratch->cap, NULL);
  return rc;
}

int vs_rec_retire_both(vs_ctx *ctx, VsRecBlock *blk, VsRecBlock *scratch, hipError_t launched)
{
  const int rc = vs_rec_retire(ctx, blk, launched);
  const int rc2 = vs_rec_retire(ctx, scratch, launched);
  return rc != VS_OK ? rc : rc2;
}

#endif
