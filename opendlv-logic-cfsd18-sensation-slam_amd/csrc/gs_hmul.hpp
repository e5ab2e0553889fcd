// gs_hmul.hpp — y = H v on the device, H the block-sparse system the last linearisation left in HBM (gs_multiply_hessian, and the two
// products of a dogleg trial).  DevGraph and gs_kernels.hip do not know about it: the kernels of gs_hmul.hip only READ the stored blocks.
//
// v and y are in vertex order: poses [N + tN][3] (a grown plan's tail poses behind the base ones, as in dpose), landmarks [M + tM][2]
// (as in dlm).  Rows of fixed vertices come out as exact zeros; their columns do not count either, because the linearisation stores a
// zero block wherever an endpoint is fixed.
#pragma once
#include "gs_device.hpp"

namespace gs {

// asynchronous on st; v_* and y_* are device pointers, y must not alias v
void launch_hmul(const DevGraph &d, const double *v_pose, const double *v_lm, double *y_pose, double *y_lm, hipStream_t st);

}  // namespace gs
