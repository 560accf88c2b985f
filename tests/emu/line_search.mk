# the keep rule of the one-trajectory builds' line search under the lane emulator, with a driver of its own
# (tsat_emu_line_search.cpp); built by tests/line_search_common.py when a test first asks for it:
#   make -C tests/emu -f line_search.mk libtsat_emu_line_search.so libtsat_emu_line_search_dense.so
# Flags as the emulator Makefile's (-ffp-contract=off pins the order of the floating-point operations).
CXX ?= g++
CSRC = ../../tortoisesat.jl_amd/csrc
FLAGS = -O2 -std=c++20 -fPIC -pthread -march=x86-64-v3 -ffp-contract=off -shared
DEP = tsat_emu_line_search.cpp tsat_emu.cpp $(CSRC)/tsat_packed.hpp $(CSRC)/tsat_device.hpp $(CSRC)/tsat_host_pack.hpp ../../include/tortoise_hip.h
libtsat_emu_line_search.so: $(DEP)
	$(CXX) $(FLAGS) -o $@ tsat_emu_line_search.cpp
libtsat_emu_line_search_dense.so: $(DEP)
	$(CXX) $(FLAGS) -DTSAT_DENSE -o $@ tsat_emu_line_search.cpp
