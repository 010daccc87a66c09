/* stand-in for <cuda.h>: see ref_host.h */
#include "ref_host.h"
