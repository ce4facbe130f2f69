# Top-level build of the MI355X (gfx950) numerics library and the C++ host layer.
# `make -j8` (also driven by __graft_entry__.build()).
HIPCC    ?= /opt/rocm/bin/hipcc
CXX      ?= g++
ARCH     ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -Wno-unused-result -Wno-unused-value
BUILD    := build
LIBDIR   := gpr_amd/lib

HIP_SRCS := $(wildcard gpr_amd/csrc/*.hip)
CPP_SRCS := $(wildcard gpr_amd/csrc/*.cpp)
HIP_OBJS := $(patsubst gpr_amd/csrc/%.hip,$(BUILD)/%.o,$(HIP_SRCS))
CPP_OBJS := $(patsubst gpr_amd/csrc/%.cpp,$(BUILD)/%.o,$(CPP_SRCS))
HDRS     := $(wildcard gpr_amd/csrc/*.h) include/gprx.h

HOST_SRCS := $(wildcard gpr_amd/host/*.cpp)
HOST_HDRS := $(wildcard include/gpr/*.h) include/gprx.h
CXXFLAGS  ?= -O2 -std=c++17 -fPIC -Wall -pthread -Iinclude
CPPTESTS  := $(LIBDIR)/gp_host_test $(LIBDIR)/host_cpu_test $(LIBDIR)/gp_append_test $(LIBDIR)/pt_sched_test \
             $(LIBDIR)/matern_cpu_test $(LIBDIR)/gp_matern_test $(LIBDIR)/gp_remove_test $(LIBDIR)/loo_test \
             $(LIBDIR)/sample_test $(LIBDIR)/ard_test $(LIBDIR)/sparse_reuse_test

all: $(LIBDIR)/libgprx.so $(LIBDIR)/libgpr_amd.so cpptests oracle

# The VALU fallback build and gradient (k_build.hip, k_lml.hip) ask for a full unroll of their
# 4 x 4 store / reduce loops around the inlined kernel-tree evaluation; its size exceeds LLVM's
# default pragma budget (the request was silently dropped: -Wpass-failed), so it is raised for
# these two files (fewer VGPRs, no scratch: the loop indices stay compile-time register indices).
$(BUILD)/k_build.o $(BUILD)/k_lml.o $(BUILD)/codeobj/k_build.elf $(BUILD)/codeobj/k_lml.elf: \
	HIPFLAGS += -mllvm -pragma-unroll-threshold=200000

$(BUILD)/%.o: gpr_amd/csrc/%.hip $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(BUILD)/%.o: gpr_amd/csrc/%.cpp $(HDRS) | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIBDIR)/libgprx.so: $(HIP_OBJS) $(CPP_OBJS) | $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^ -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

# C++ host API (GaussianProcess<T>, Kernel<T>, Likelihood<T>) over libgprx
$(LIBDIR)/libgpr_amd.so: $(HOST_SRCS) $(HOST_HDRS) $(LIBDIR)/libgprx.so
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRCS) -L$(LIBDIR) -lgprx -Wl,-rpath,'$$ORIGIN'

cpptests: $(CPPTESTS)

$(LIBDIR)/%: tests/cpp/%.cpp $(HOST_HDRS) $(LIBDIR)/libgpr_amd.so
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(LIBDIR) -lgpr_amd -lgprx -Wl,-rpath,'$$ORIGIN'

# The schedule planner alone (host C++: no libgprx, no HIP runtime) under its stand-alone test
# program; `make pt_sched_asan` builds the same two sources with the address and undefined-
# behaviour sanitizers and runs the program (a CPU check: not part of `all`)
PT_SCHED_SRCS  := tests/cpp/pt_sched_test.cpp gpr_amd/csrc/pt_sched.cpp
PT_SCHED_HDRS  := gpr_amd/csrc/pt_sched.h gpr_amd/csrc/gprx_error.h include/gprx.h
PT_SCHED_FLAGS := -O2 -g -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include

$(LIBDIR)/pt_sched_test: $(PT_SCHED_SRCS) $(PT_SCHED_HDRS) | $(LIBDIR)
	$(CXX) $(PT_SCHED_FLAGS) -o $@ $(PT_SCHED_SRCS)

pt_sched_asan: $(PT_SCHED_SRCS) $(PT_SCHED_HDRS) | $(BUILD)
	$(CXX) $(PT_SCHED_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
		-o $(BUILD)/pt_sched_test_asan $(PT_SCHED_SRCS)
	$(BUILD)/pt_sched_test_asan

# `make codeobj`: the device side of every source alone, with the file's own flags and a fixed
# compilation-unit id (without one the ELF carries a symbol hashed from the file's path and text),
# then one line per file of sha256 hashes: the whole ELF, .text, .rodata (the kernel descriptors)
# and the notes (the amdhsa metadata: VGPR / SGPR / spill counts, LDS sizes).  A pure refactor of
# a kernel file leaves the listing as its parent's: run it in both checkouts and diff.  It only
# hashes; it needs no GPU and is not part of `all`.
LLVMBIN  ?= $(dir $(HIPCC))../llvm/bin
CODEOBJ  := $(BUILD)/codeobj
CO_FLAGS := --offload-device-only --no-gpu-bundle-output -cuid=gprx
CO_ELFS  := $(sort $(patsubst gpr_amd/csrc/%.hip,$(CODEOBJ)/%.elf,$(HIP_SRCS)) \
                   $(patsubst gpr_amd/csrc/%.cpp,$(CODEOBJ)/%.elf,$(CPP_SRCS)))

$(CODEOBJ)/%.elf: gpr_amd/csrc/%.hip $(HDRS) | $(CODEOBJ)
	$(HIPCC) $(HIPFLAGS) $(CO_FLAGS) -c $< -o $@

$(CODEOBJ)/%.elf: gpr_amd/csrc/%.cpp $(HDRS) | $(CODEOBJ)
	$(HIPCC) $(HIPFLAGS) $(CO_FLAGS) -x hip -c $< -o $@

codeobj: $(CO_ELFS)
	@printf '%-18s %-16s %-16s %-16s %-16s\n' file elf .text .rodata notes; \
	h() { sha256sum | cut -c1-16; }; \
	for f in $(CO_ELFS); do \
	  for s in text rodata; do $(LLVMBIN)/llvm-objcopy -O binary --only-section=.$$s $$f $$f.$$s; done; \
	  printf '%-18s %s %s %s %s\n' $$(basename $$f .elf) $$(h < $$f) $$(h < $$f.text) $$(h < $$f.rodata) \
	    $$($(LLVMBIN)/llvm-readelf --notes $$f | h); \
	done

# `make codeobj-kernels`: the same ELFs, one line per kernel instead of per file, so that a
# kernel that changes files (or loses a neighbour) can still be compared with its parent: the
# mangled name, the file, a sha256 hash of the kernel's instruction text (its disassembly without
# the `// address: encoding` comments, the symbol's address line and the `...` that stands for
# the zero padding after a file's last kernel, which is layout and not code) and its amdhsa
# metadata entry: VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, SGPR and VGPR spills.  Sorted by name:
# two checkouts diff cleanly when the file column is ignored.  It only hashes and prints.
codeobj-kernels: $(CO_ELFS)
	@printf '%s %s %s %s\n' kernel file text 'vgpr agpr sgpr lds scratch sgpr_spill vgpr_spill'; \
	for f in $(CO_ELFS); do \
	  $(LLVMBIN)/llvm-readelf --notes $$f | awk ' \
	    /^  - \.agpr_count:/ { ag = $$3 } \
	    /^    \.group_segment_fixed_size:/ { lds = $$2 } \
	    /^    \.private_segment_fixed_size:/ { scr = $$2 } \
	    /^    \.sgpr_count:/ { sg = $$2 } \
	    /^    \.sgpr_spill_count:/ { ss = $$2 } \
	    /^    \.symbol:/ { sym = $$2; sub(/\.kd$$/, "", sym) } \
	    /^    \.vgpr_count:/ { vg = $$2 } \
	    /^    \.vgpr_spill_count:/ { vs = $$2 } \
	    /^    \.wavefront_size:/ { print sym, vg, ag, sg, lds, scr, ss, vs }' | \
	  while read -r sym meta; do \
	    printf '%s %s %s %s\n' $$sym $$(basename $$f .elf) \
	      $$($(LLVMBIN)/llvm-objdump -d --disassemble-symbols=$$sym $$f | grep '^[[:space:]]' | \
	         sed -e 's|[[:space:]]*//.*$$||' -e '/^[[:space:]]*\.\.\.$$/d' | sha256sum | cut -c1-16) "$$meta"; \
	  done; \
	done | sort

oracle:
	$(MAKE) -s -C oracle

$(BUILD) $(LIBDIR) $(CODEOBJ):
	mkdir -p $@

clean:
	rm -rf $(BUILD) $(LIBDIR)/*.so $(CPPTESTS)
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean cpptests pt_sched_asan codeobj codeobj-kernels
