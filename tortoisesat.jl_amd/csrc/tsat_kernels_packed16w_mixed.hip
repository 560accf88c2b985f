// tsat_kernels_packed16w_mixed.hip — the unit of one build of the solve kernel: packed16w, mixed precision (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 6
#define TSAT_JAC32 1
#include "tsat_kernels_packed.hip"
