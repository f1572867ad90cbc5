/*
 * vs_kernels.hip -- the launchers of the synthesis kernels.  The kernels stand in a file per family, each with the table
 * of its instantiations (vs_kernel_table.h): vs_synth_one_wave.hip (built twice: 64 and 16 utterances per wavefront),
 * vs_synth_ws.hip, vs_out_noise.hip, vs_filter_wide.hip; vs_selftest.hip brings its own three launchers.
 *
 * Which kernel a launch runs, with what block, grid and LDS, is decided in csrc/vs_planhost.c (vs_launch_pick and its
 * kin: device-free, held on the CPU by tests/c/test_planhost_asan.c).  Here: launchers that ask, look the identifier up
 * in the table of its family and launch.
 */
#include "vs_kernel_table.h"

static const VsKernelEntry *vs_family_table(int family)
{
  switch (family) {
  case VS_KF_ONE_WAVE: return vs_kernel_table_one_wave;
  case VS_KF_NARROW: return vs_kernel_table_narrow;
  case VS_KF_WS:
  case VS_KF_WS_POW: return vs_kernel_table_ws;
  case VS_KF_WIDE: return vs_kernel_table_wide;
  case VS_KF_OUT_POWER:
  case VS_KF_OUT_POWER_FILL: return vs_kernel_table_out_power;
  default: return nullptr;
  }
}

static hipError_t vs_launch_picked(const VsLaunchPick &pick, const VsKernelArgs *args, hipStream_t stream)
{
  const VsKernelEntry *e = vs_family_table(VS_KERNEL_FAMILY(pick.kernel));
  if (!e) return hipErrorInvalidValue;
  while (e->fn && e->id != pick.kernel) ++e;
  if (!e->fn) return hipErrorInvalidValue;
  if (pick.lds_bytes > 48 * 1024) {
    hipError_t err = hipFuncSetAttribute((const void *)e->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pick.lds_bytes);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(e->fn, dim3(pick.grid), dim3(pick.block), pick.lds_bytes, stream, *args);
  return hipGetLastError();
}

extern "C" hipError_t vs_launch_kernel(int arith, int kind, bool log, bool wave_specialised, bool pre1,
                                       const VsKernelArgs *args, unsigned grid, size_t lds_bytes, hipStream_t stream)
{
  VsLaunchPick pick;
  if (vs_launch_pick(arith, kind, log, wave_specialised, pre1, args, grid, lds_bytes, &pick) != 0) return hipErrorInvalidValue;
  return vs_launch_picked(pick, args, stream);
}

extern "C" hipError_t vs_launch_kernel_narrow(int arith, int kind, bool log, bool pre1, const VsKernelArgs *args,
                                              unsigned grid, size_t lds_bytes, hipStream_t stream)
{
  VsLaunchPick pick;
  if (vs_launch_pick_narrow(arith, kind, log, pre1, grid, lds_bytes, &pick) != 0) return hipErrorInvalidValue;
  return vs_launch_picked(pick, args, stream);
}

extern "C" hipError_t vs_launch_filter_wide(int arith, const VsKernelArgs *args, unsigned grid, hipStream_t stream)
{
  VsLaunchPick pick;
  if (vs_launch_pick_wide(arith, args, grid, &pick) != 0) return hipErrorInvalidValue;
  return vs_launch_picked(pick, args, stream);
}

extern "C" hipError_t vs_launch_out_noise(const VsKernelArgs *args, hipStream_t stream)
{
  VsOutNoisePick pick;
  if (vs_launch_pick_out_noise(args, vs_noise_table.octets, vs_noise_table.row_major, &pick) != 0) return hipErrorInvalidValue;
  const hipError_t err = vs_launch_picked(pick.power, args, stream);
  if (err != hipSuccess) return err;
  vs_noise_fn fn = nullptr;
  for (const auto &n : vs_noise_table.e)
    if (n.id == pick.noise.kernel) fn = n.fn;
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3(pick.noise.grid, pick.noise_grid_y), dim3(pick.noise.block), 0, stream, *args, pick.segs,
                     pick.seg_magic, pick.seg_shift);
  return hipGetLastError();
}
