// Explicit instantiations of the polyphase launchers (conv_bf16_kernel.h, TAPS = 4), f16.
#include "conv_bf16_kernel.h"

namespace loco {
template void launch_poly_b<PR_F16>(const ConvArgs&, hipStream_t);
template void launch_poly_in_b<PR_F16>(const ConvArgs&, hipStream_t);
}  // namespace loco
