// Bn254G2 instantiation of the Pippenger MSM (msm_core.cuh).
#include "msm_core.cuh"

namespace lw {
MsmCurveOps msm_ops_bn254_g2 = msm_curve_ops<Bn254G2>();
}  // namespace lw
