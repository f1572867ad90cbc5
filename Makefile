# Top-level build: the product library + drop-in CLIs (gfx950 only) and the oracle.
# Host code is C (gcc, the HIP runtime through its C API); hipcc compiles the kernels and links.
#
#   make            -> voice_synth_amd/lib/libvoicesynth.so and voice_synth_amd/bin/<each of PROGRAMS>: the drop-in CLIs
#   make oracle     -> oracle/liboracle.so and, when /root/reference exists, oracle/_ref/*
#
# -ffp-contract=off everywhere: the float/double rounding sequence is part of the parity
# contract; the fused variant of the filter uses explicit fma() calls.

ROCM    ?= /opt/rocm
HIPCC   ?= $(ROCM)/bin/hipcc
CC      ?= gcc
ARCH    ?= gfx950

PKG     := voice_synth_amd
CSRC    := $(PKG)/csrc
LIBDIR  := $(PKG)/lib
BINDIR  := $(PKG)/bin

# the synthesis kernels: a file per family (the longest compilation first); vs_kernels.hip holds their launchers
SYNTH_KERNELS := vs_synth_ws vs_synth_one_wave vs_out_noise vs_filter_wide vs_selftest
KERNEL_HDRS := $(addprefix $(CSRC)/,vs_device.h vs_planhost.h vs_kernel_table.h vs_dev_primitives.h vs_dev_generator.h vs_dev_filter.h vs_dev_onoise.h) include/voice_synth.h
# their objects; $(call synth_objs,_x): the same files built once more as vs_*_x.o (the diagnostic build, the variants)
synth_objs = $(SYNTH_KERNELS:%=$(CSRC)/%$(1).o)
ANALYSIS_CLIS := acoustic formants glottal vtrack vinverse vclosed pitch vsource vpsola
PROGRAMS := flowgen_shimmer vowel vs_batch vs_bench $(ANALYSIS_CLIS)
HIPFLAGS := -O3 --offload-arch=$(ARCH) -ffp-contract=off -fPIC -std=c++17 -Wall -Wno-unused-function
CFLAGS   := -O2 -ffp-contract=off -fno-fast-math -fPIC -Wall -Wextra -Wno-unused-parameter
HOSTFLAGS := -std=gnu11 $(CFLAGS) -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include
HOST_HDRS := $(CSRC)/vs_device.h $(CSRC)/vs_internal.h $(CSRC)/vs_planhost.h include/voice_synth.h

LIB := $(LIBDIR)/libvoicesynth.so

all: $(LIB) clis

$(LIBDIR) $(BINDIR):
	mkdir -p $@

$(CSRC)/vs_host.o: $(CSRC)/vs_host.c $(CSRC)/vs_tables.h include/voice_synth.h
	$(CC) $(CFLAGS) -c -o $@ $<

$(CSRC)/vs_kernels.o $(call synth_objs,): $(CSRC)/%.o: $(CSRC)/%.hip $(KERNEL_HDRS)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# the one-wave kernel once more with 16 utterances per wavefront: periods beyond the 64-column ring
$(CSRC)/vs_synth_one_wave_narrow.o: $(CSRC)/vs_synth_one_wave.hip $(KERNEL_HDRS)
	$(HIPCC) $(HIPFLAGS) -DVS_GROUP_LANES=16 -c -o $@ $<

# the host side of the library: plain C against the HIP runtime's C API
$(CSRC)/vs_api.o $(CSRC)/vs_blocks.o $(CSRC)/vs_delivery.o: $(CSRC)/%.o: $(CSRC)/%.c $(HOST_HDRS)
	$(CC) $(HOSTFLAGS) -c -o $@ $<

$(CSRC)/vs_planhost.o: $(CSRC)/vs_planhost.c $(CSRC)/vs_planhost.h $(CSRC)/vs_device.h include/voice_synth.h
	$(CC) -std=gnu11 $(CFLAGS) -c -o $@ $<

$(CSRC)/vs_node.o: $(CSRC)/vs_node.c $(CSRC)/vs_commguard.h $(HOST_HDRS)
	$(CC) $(HOSTFLAGS) -c -o $@ $<

$(CSRC)/vs_commguard.o: $(CSRC)/vs_commguard.c $(CSRC)/vs_commguard.h
	$(CC) -std=gnu11 $(CFLAGS) -c -o $@ $<

# the acoustic measurement, the LPC analysis, the coefficient tracks, the inverse filter, the IAIF analysis, the glottal
# parameters, the closed-phase covariance LPC, the pitch track, the guided marks, the source track, PSOLA, PSOLA with a
# time map: each its kernels and their host side
FEATURES := acoustic lpc track inverse iaif glottal cplpc pitch guided strack psola psola_ts

$(FEATURES:%=$(CSRC)/vs_%.o): $(CSRC)/vs_%.o: $(CSRC)/vs_%.hip $(CSRC)/vs_%.h include/voice_synth.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(FEATURES:%=$(CSRC)/vs_%_host.o): $(CSRC)/vs_%_host.o: $(CSRC)/vs_%_host.c $(CSRC)/vs_%.h $(HOST_HDRS)
	$(CC) $(HOSTFLAGS) -c -o $@ $<

# the inverse filter walks the sets as the coefficient tracks do: their classes and LDS plan
$(CSRC)/vs_inverse.o $(CSRC)/vs_inverse_host.o: $(CSRC)/vs_track.h
# IAIF runs on the LPC analysis's frames, records and root phase
$(CSRC)/vs_iaif.o $(CSRC)/vs_iaif_host.o: $(CSRC)/vs_lpc.h
$(CSRC)/vs_iaif.o $(CSRC)/vs_lpc.o: $(CSRC)/vs_lpc_roots.h
# the closed-phase analysis too: the LPC analysis's row records, frames and root phase
$(CSRC)/vs_cplpc.o $(CSRC)/vs_cplpc_host.o: $(CSRC)/vs_lpc.h
$(CSRC)/vs_cplpc.o: $(CSRC)/vs_lpc_roots.h
# the pitch track's candidate kernel runs the period kernel's correlation core on the period kernel's LDS plan
$(CSRC)/vs_acoustic.o $(CSRC)/vs_pitch.o: $(CSRC)/vs_ac_corr.h
$(CSRC)/vs_pitch.o $(CSRC)/vs_pitch_host.o: $(CSRC)/vs_acoustic.h
# the source track's kernel draws and converts with the synthesis kernels' primitives
$(CSRC)/vs_strack.o: $(CSRC)/vs_dev_primitives.h $(CSRC)/vs_device.h
# PSOLA with a time map cuts the output into PSOLA's tiles and embeds its common launch arguments; its host side calls
# vs_psola_host.c's common refusals, argument fill and host parts (the library links both)
$(CSRC)/vs_psola_ts.o $(CSRC)/vs_psola_ts_host.o: $(CSRC)/vs_psola.h
# the kernels of both share their target, run check and overlap-add core
$(CSRC)/vs_psola.o $(CSRC)/vs_psola_ts.o: $(CSRC)/vs_psola_dev.h
# the three kernels that write vs_lpc_frame records: the row of a frame, Levinson-Durbin, the set store, the record
$(CSRC)/vs_lpc.o $(CSRC)/vs_iaif.o $(CSRC)/vs_cplpc.o: $(CSRC)/vs_lpc_frame.h

# what every build of the library links; the diagnostic build and the variants bring their own synthesis kernel objects
LIB_OBJS := $(call synth_objs,) $(addprefix $(CSRC)/,vs_host.o vs_planhost.o vs_kernels.o vs_synth_one_wave_narrow.o vs_api.o vs_blocks.o \
              vs_delivery.o vs_node.o vs_commguard.o $(foreach f,$(FEATURES),vs_$(f).o vs_$(f)_host.o))
lib_objs_with = $(call synth_objs,$(1)) $(filter-out $(call synth_objs,),$(LIB_OBJS))
LINK_LIB = $(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(1) $(2) -lm -lpthread -ldl

$(LIB): $(LIB_OBJS) | $(LIBDIR)
	$(call LINK_LIB,$@,$^)

clis: $(addprefix $(BINDIR)/,$(PROGRAMS))

$(BINDIR)/%: $(PKG)/cli/%.c $(PKG)/cli/cli_common.h $(LIB) | $(BINDIR)
	$(CC) -O2 -ffp-contract=off -Wall -Iinclude -o $@ $< -L$(LIBDIR) -lvoicesynth -lm -lpthread -Wl,-rpath,'$$ORIGIN/../lib'
# the analysis programs share their batch, their option blocks and the filter tools' scaffold
$(addprefix $(BINDIR)/,$(ANALYSIS_CLIS)): $(PKG)/cli/cli_analysis.h

oracle:
	$(MAKE) -C oracle all

# resource usage (VGPR/SGPR/LDS/occupancy) of every kernel
resources: $(SYNTH_KERNELS:%=resources-%)
resources-%:
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o /dev/null $(CSRC)/$*.hip

clean:
	rm -f $(CSRC)/*.o $(LIB) $(LIBDIR)/libvoicesynth_*.so $(addprefix $(BINDIR)/,$(PROGRAMS))
	$(MAKE) -C oracle clean

.PHONY: all clis oracle resources clean diag variant isa

# A/B variants of the library for same-box comparisons (tools/gpu_ab.sh): the synthesis kernels compiled with $(DEFS)
#   make variant NAME=sleep2 DEFS="-DVS_POLL_SLEEP=2"   ->  lib/libvoicesynth_sleep2.so   (select with VS_LIB)
variant: $(LIBDIR)/libvoicesynth_$(NAME).so
# (compiled anew every time: the same NAME may come back with other DEFS)
$(call synth_objs,_$(NAME)): $(CSRC)/%_$(NAME).o: $(CSRC)/%.hip FORCE
	$(HIPCC) $(HIPFLAGS) $(DEFS) -c -o $@ $<
FORCE:
$(LIBDIR)/libvoicesynth_$(NAME).so: $(call lib_objs_with,_$(NAME)) | $(LIBDIR)
	$(call LINK_LIB,$@,$^)

# diagnostic build with s_memtime stamps (never shipped, never timed): tools/diag_bench.py
diag:
	$(MAKE) variant NAME=diag DEFS=-DVS_DIAG

# device listings of the shipped kernels (same flags), one per file, for tools/isa_loops.py
isa: $(SYNTH_KERNELS:%=build/%.s)
build/%.s: $(CSRC)/%.hip $(KERNEL_HDRS) Makefile
	mkdir -p build && $(HIPCC) $(HIPFLAGS) -Iinclude -I$(CSRC) -S --cuda-device-only -o $@ $<
