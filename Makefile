# Plain-make build of the C-ABI library and the C host program, for users who do not want
# Python in the loop (python -m adsbdec_amd._build runs the same commands; keep them in step).
# hipcc cross-compiles the gfx950 code object without a GPU.
HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
ROCM     ?= /opt/rocm
# -ffp-contract=off: the reference arithmetic is binary32 multiply THEN add
# -amdgpu-atomic-optimizer-strategy=None: see adsbdec_amd/_build.py (the LDS survivor-queue atomics stay per lane)
HIPFLAGS ?= --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wall -Wno-unused-function -mllvm -amdgpu-atomic-optimizer-strategy=None -Xarch_host -mavx2
CSRC     := adsbdec_amd/csrc
LIBDIR   := adsbdec_amd/lib
LIB      := $(LIBDIR)/libadsbdec_amd.so
CLI      := $(LIBDIR)/adsbdec_amd_cli
# dependencies: every compile writes <object>.d (-MMD), included at the bottom -- no hand-kept header list to forget a file in

all: $(LIB) $(CLI)

$(LIBDIR)/%.hip.o: $(CSRC)/%.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -MMD -MF $@.d -c $< -o $@

$(LIBDIR)/format.c.o: $(CSRC)/format.c
	@mkdir -p $(LIBDIR)
	$(CC) -O2 -fPIC -Wall -MMD -MF $@.d -c $< -o $@

$(LIBDIR)/%.cpp.o: $(CSRC)/%.cpp
	@mkdir -p $(LIBDIR)
	g++ -O2 -fPIC -std=c++17 -Wall -Wextra -pthread -MMD -MF $@.d -c $< -o $@

$(LIB): $(LIBDIR)/scan_kernel.hip.o $(LIBDIR)/scan_batch_kernel.hip.o $(LIBDIR)/scan_iq_kernel.hip.o $(LIBDIR)/scan_iq8_kernel.hip.o $(LIBDIR)/scan_power_kernel.hip.o $(LIBDIR)/seam_kernel.hip.o $(LIBDIR)/decoder.hip.o $(LIBDIR)/decoder_collect.hip.o $(LIBDIR)/decoder_lifecycle.hip.o $(LIBDIR)/decoder_batch.hip.o $(LIBDIR)/decoder_shard.hip.o $(LIBDIR)/unpack12.hip.o $(LIBDIR)/unpack12_batch.hip.o $(LIBDIR)/convert_samples.hip.o $(LIBDIR)/power_export_kernel.hip.o $(LIBDIR)/decoder_export.hip.o $(LIBDIR)/power_export_batch_kernel.hip.o $(LIBDIR)/decoder_export_batch.hip.o $(LIBDIR)/level_kernel.hip.o $(LIBDIR)/decoder_level.hip.o $(LIBDIR)/level_batch_kernel.hip.o $(LIBDIR)/decoder_level_batch.hip.o $(LIBDIR)/level_windows_kernel.hip.o $(LIBDIR)/decoder_level_windows.hip.o $(LIBDIR)/decoder_stage.hip.o $(LIBDIR)/decoder_flavour.hip.o $(LIBDIR)/burst_kernel.hip.o $(LIBDIR)/burst_slice_kernel.hip.o $(LIBDIR)/decoder_bursts.hip.o $(LIBDIR)/gather_kernel.hip.o $(LIBDIR)/decoder_gather.hip.o $(LIBDIR)/gather_pack12_kernel.hip.o $(LIBDIR)/decoder_gather_pack12.hip.o $(LIBDIR)/format.c.o $(LIBDIR)/multi.cpp.o $(LIBDIR)/host_abi.cpp.o $(LIBDIR)/numa.cpp.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $^ -lm -lpthread

# the host program (_build.py CLI_SOURCES): one line over all its sources, rebuilt when any of them or a header beside them changes
CLI_SRCS := $(addprefix $(CSRC)/cli/,adsbdec_amd_cli.c options.c common.c stream.c batch.c export.c level.c bursts.c record.c sink.c burst_archive.c)
$(CLI): $(CLI_SRCS) $(wildcard $(CSRC)/cli/*.h) $(LIB) include/adsbdec_amd.h
	$(CC) -O2 -Wall -D__HIP_PLATFORM_AMD__ -o $@ $(CLI_SRCS) -Iinclude -I$(ROCM)/include -L$(LIBDIR) -ladsbdec_amd -L$(ROCM)/lib -lamdhip64 -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(ROCM)/lib

# test infrastructure (never linked into the library): the CPU oracle, and the reference
# objects it is pinned against when /root/reference is present
oracle:
	$(MAKE) -C oracle

check: all
	python -m pytest tests -q -m "not gpu"

clean:
	rm -f $(LIBDIR)/*.o $(LIBDIR)/*.o.d $(LIB) $(CLI)

-include $(wildcard $(LIBDIR)/*.o.d)

.PHONY: all oracle check clean
