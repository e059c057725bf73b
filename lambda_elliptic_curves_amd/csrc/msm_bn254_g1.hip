// Bn254G1 instantiation of the Pippenger MSM (msm_core.cuh).
#include "msm_core.cuh"

namespace lw {
MsmCurveOps msm_ops_bn254_g1 = msm_curve_ops<Bn254G1>();
}  // namespace lw
