/* stand-in for <torch/extension.h>: see ../ref_host.h */
#include "../ref_host.h"
