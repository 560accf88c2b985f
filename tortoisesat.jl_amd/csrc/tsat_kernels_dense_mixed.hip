// tsat_kernels_dense_mixed.hip — the unit of one build of the solve kernel: dense, mixed precision (the table of builds at the head of tsat_device.hpp)
#define TSAT_BUILD 2
#define TSAT_JAC32 1
#include "tsat_kernels_dense.hip"
