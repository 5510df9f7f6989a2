// What fixed_point.hip uses of the numpy-order passes (numpy_order.hip).
#pragma once

#include "fixed_point.h"

namespace irlmx {
// Whether every ELL row holds its nonzero entries in ascending column order
// (np_ell_ascending_kernel), into *sorted; synchronises the stream.
int ell_rows_sorted(const Model& m, hipStream_t st, bool* sorted);
}  // namespace irlmx
