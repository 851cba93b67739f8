// agx_proximity.hip -- the closest-point query behind agx_proximity (include/agx.h): stage B, after the variant's frames kernel.  Variant
// independent, like the ray caster of csrc/agx_render.hip.  One workgroup = one wavefront; the mapping of (environment, pair) items to lanes,
// the record and the reduction to nearest records are described in csrc/agx_proximity.h, which holds the body.
#include "agx_wave.h"
#include "agx_proximity.h"

extern "C" __global__ void __launch_bounds__(64)
agx_proximity_kernel(const agx_prox_args A) {
  agxprox::prox_wave(A, (int)blockIdx.x, (int)threadIdx.x);
}

void agx_launch_proximity(hipStream_t st, const agx_prox_args& A) {
  const int per_wave = AGX_WAVE / A.group;
  hipLaunchKernelGGL(agx_proximity_kernel, dim3((A.count + per_wave - 1) / per_wave), dim3(64), 0, st, A);
}
