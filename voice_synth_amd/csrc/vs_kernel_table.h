/*
 * vs_kernel_table.h -- what the files of synthesis kernels and the launchers of vs_kernels.hip share: the headers all of
 * them stand on and the tables the launchers look a kernel up in.  A file ends with the table of the kernels it
 * instantiates: an entry's identifier (vs_planhost.h) and its pointer are written by one macro, in that file, from one
 * spelling of the template arguments.
 */
#ifndef VS_KERNEL_TABLE_H
#define VS_KERNEL_TABLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/voice_synth.h"
#include "vs_device.h"
#include "vs_planhost.h"

#include "vs_dev_primitives.h"

typedef void (*vs_kernel_fn)(VsKernelArgs);
struct VsKernelEntry {
  int id; /* VS_KERNEL_ID */
  vs_kernel_fn fn;
};
/* (the noise pass takes its geometry behind the arguments; what its build was compiled for comes with its table) */
typedef void (*vs_noise_fn)(VsKernelArgs, unsigned, unsigned, unsigned);
struct VsNoiseTable {
  int octets, row_major; /* VS_ONOISE_OCTETS, VS_ONOISE_ROWMAJOR */
  struct {
    int id;
    vs_noise_fn fn;
  } e[2];
};

extern "C" {
/* by family (VS_KERNEL_FAMILY); each ends with {0, nullptr} */
extern const VsKernelEntry vs_kernel_table_one_wave[], vs_kernel_table_narrow[]; /* vs_synth_one_wave.hip, its two builds */
extern const VsKernelEntry vs_kernel_table_ws[];                                 /* vs_synth_ws.hip */
extern const VsKernelEntry vs_kernel_table_wide[];                               /* vs_filter_wide.hip */
extern const VsKernelEntry vs_kernel_table_out_power[];                          /* vs_out_noise.hip */
extern const VsNoiseTable vs_noise_table;
}

#endif
