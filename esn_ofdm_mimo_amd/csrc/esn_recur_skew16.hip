// Instantiations of the 16x16x32 skewed predict kernel (esn_recur_skew16_impl.h).
#include "esn_recur_skew16_impl.h"
#include "esn_launch.h"

namespace esn {

int launch_recur_skew16(int precision, const RecurParams& p, hipStream_t stream, bool io32) {
    if (precision == ESN_F16) return io32 ? launch_skew16<TraitsF16, true>(p, stream) : launch_skew16<TraitsF16, false>(p, stream);
    if (precision == ESN_BF16) return io32 ? launch_skew16<TraitsBF16, true>(p, stream) : launch_skew16<TraitsBF16, false>(p, stream);
    return -1;
}

}  // namespace esn
