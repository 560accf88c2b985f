// tsat_kernels_packed8w.hip — the unit of one build of the solve kernel: packed8w (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 5
#include "tsat_kernels_packed.hip"
