// Bls12381G1 instantiation of the Pippenger MSM (msm_core.cuh).
#include "msm_core.cuh"

namespace lw {
MsmCurveOps msm_ops_bls12381_g1 = msm_curve_ops<Bls12381G1>();
}  // namespace lw
