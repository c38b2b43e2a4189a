/* explicit instantiations, see kmr_instances.hpp: this one file is compiled once per group and key width, the Makefile
 * passes -DKMR_INST_<GROUP> (SKX, SKC, EX, PART) and -DKMR_INST_W=<key words> for the object build/kmr_inst_<group><w>.o */
#include <hip/hip_runtime.h>
#if !defined(KMR_INST_W) || (defined(KMR_INST_SKX) + defined(KMR_INST_SKC) + defined(KMR_INST_EX) + defined(KMR_INST_PART) != 1)
#error "kmr_inst.hip wants exactly one of -DKMR_INST_SKX / _SKC / _EX / _PART and -DKMR_INST_W=1..4"
#endif
#define KMR_INSTANCE_TU      /* the plain (non-template) kernels of the headers belong to kmr_api.hip */
#include "kmr_instances.hpp"
