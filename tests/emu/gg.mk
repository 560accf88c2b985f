# the gravity-gradient ensemble and hold (tsat_tvlqr_ensemble_gg, tsat_mpc_run_held_gg) under the lane emulator, with a driver of
# their own (tsat_emu_gg.cpp); built by tests/gg_common.py when a test first asks for it:
#   make -C tests/emu -f gg.mk libtsat_emu_gg.so
# Flags as the emulator Makefile's (-ffp-contract=off pins the order of the floating-point operations).
CXX ?= g++
CSRC = ../../tortoisesat.jl_amd/csrc
FLAGS = -O2 -std=c++20 -fPIC -pthread -march=x86-64-v3 -ffp-contract=off -shared
libtsat_emu_gg.so: tsat_emu_gg.cpp tsat_emu.cpp $(CSRC)/tsat_gg.hpp $(CSRC)/tsat_mpc_held.hpp $(CSRC)/tsat_mpc_dispersed.hpp $(CSRC)/tsat_dispersed.hpp $(CSRC)/tsat_ensemble.hpp $(CSRC)/tsat_packed.hpp $(CSRC)/tsat_device.hpp $(CSRC)/tsat_host_pack.hpp ../../include/tortoise_hip.h
	$(CXX) $(FLAGS) -o $@ tsat_emu_gg.cpp
