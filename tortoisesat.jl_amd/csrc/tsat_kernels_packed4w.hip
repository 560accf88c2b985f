// tsat_kernels_packed4w.hip — the unit of one build of the solve kernel: packed4w (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 7
#include "tsat_kernels_packed.hip"
