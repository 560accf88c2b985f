# the dispersed-plant ensemble kernel under the CPU lane emulator (test infrastructure; see tsat_emu_dispersed.cpp): make -f dispersed.mk
CXX ?= g++
C = ../../tortoisesat.jl_amd/csrc
DEP = tsat_emu_dispersed.cpp tsat_emu.cpp $(C)/tsat_dispersed.hpp $(C)/tsat_ensemble.hpp $(C)/tsat_device.hpp $(C)/tsat_host_pack.hpp ../../include/tortoise_hip.h
# the flags of the other emulator builds (Makefile): the order of the floating-point operations is the source's, nothing is fused
FLAGS = -O2 -std=c++20 -fPIC -pthread -march=x86-64-v3 -ffp-contract=off -shared
libtsat_emu_dispersed.so: $(DEP)
	$(CXX) $(FLAGS) -o $@ tsat_emu_dispersed.cpp
clean:
	rm -f libtsat_emu_dispersed.so
