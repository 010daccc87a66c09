/* stand-in for <cuda_runtime.h>: see ref_host.h */
#include "ref_host.h"
