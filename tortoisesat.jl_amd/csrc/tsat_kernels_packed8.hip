// tsat_kernels_packed8.hip — the unit of one build of the solve kernel: packed8 (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 4
#include "tsat_kernels_packed.hip"
