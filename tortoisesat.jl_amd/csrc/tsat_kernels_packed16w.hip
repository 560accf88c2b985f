// tsat_kernels_packed16w.hip — the unit of one build of the solve kernel: packed16w (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 6
#include "tsat_kernels_packed.hip"
