// The pose-ambiguity instantiations of k_light.hip in a module of their own (see that file's header):
// light_extract_kernel<*, true> behind launch_light_extract_alt.  Compiled with -ffp-contract=off like k_light.hip.
#define IRMV_ALT_TU 1
#include "k_light.hip"

namespace irmv {
template __global__ void light_extract_kernel<true, true>(LightArgs a);
template __global__ void light_extract_kernel<false, true>(LightArgs a);
}
