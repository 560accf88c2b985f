# the held re-planning loop fed measurements (tsat_mpc_run_held_sensed) under the lane emulator, with a driver of its own
# (tsat_emu_mpc_sensed.cpp); built by tests/mpc_sensed_common.py when a test first asks for it:
#   make -C tests/emu -f mpc_sensed.mk libtsat_emu_mpc_sensed.so
# Flags as the emulator Makefile's (-ffp-contract=off pins the order of the floating-point operations).
CXX ?= g++
CSRC = ../../tortoisesat.jl_amd/csrc
FLAGS = -O2 -std=c++20 -fPIC -pthread -march=x86-64-v3 -ffp-contract=off -shared
libtsat_emu_mpc_sensed.so: tsat_emu_mpc_sensed.cpp tsat_emu.cpp $(CSRC)/tsat_mpc_sensed.hpp $(CSRC)/tsat_sensed.hpp $(CSRC)/tsat_pd.hpp $(CSRC)/tsat_gg.hpp $(CSRC)/tsat_mpc_held.hpp $(CSRC)/tsat_mpc_dispersed.hpp $(CSRC)/tsat_dispersed.hpp $(CSRC)/tsat_ensemble.hpp $(CSRC)/tsat_packed.hpp $(CSRC)/tsat_device.hpp $(CSRC)/tsat_host_pack.hpp ../../include/tortoise_hip.h
	$(CXX) $(FLAGS) -o $@ tsat_emu_mpc_sensed.cpp
