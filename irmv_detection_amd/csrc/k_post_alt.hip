// The pose-ambiguity instantiations of k_post.hip in a module of their own (see that file's header): nms_pnp_kernel<true>
// behind launch_nms_pnp_alt, and the two-solution PnP kernel of irmv_pnp_solve2.  Compiled with -ffp-contract=off like k_post.hip.
#define IRMV_ALT_TU 1
#include "k_post.hip"

namespace irmv {
template __global__ void nms_pnp_kernel<true>(PostArgs a);
}
