// The one loop that launches the passes of a transform, for the 256-bit fields (ntt256.hip), BabyBear (ntt_bb.hip) and the tile
// families (tile_pass.cuh): it walks a PassSchedule (ntt_plan.h), stages an in-place single pass, hands each pass its buffers, strides
// and grid and wraps the launch in its profile line and error check.  What differs per field is the `launch` callable.
#pragma once
#include "internal.h"
#include "ntt_plan.h"

namespace lw {

// `batch` columns of 2^Lw words: the caller's `in_stride` / `out_stride` words apart in d_in / d_out (words of
// `word_bytes` each), dense in `work`, which holds batch x 2^Lw caller words and is only touched when there is more than
// one pass or d_in == d_out.  launch(step, in, out, in_stride, out_stride, grid), strides in words between the columns of
// the batch, fills the field's parameters, launches its kernel and returns the name of the pass's line in lw_hip_profile_end.
template <class Launch>
static int run_passes(Context &c, const PassSchedule &sc, uint32_t Lw, const void *d_in, uint64_t in_stride, void *d_out, uint64_t out_stride,
                      uint32_t batch, void *work, size_t word_bytes, hipStream_t stream, Launch launch) {
    const uint64_t nw = 1ull << Lw;
    if (sc.stage)   // the last pass permutes across tiles
        LW_HIP_CHECK(hipMemcpy2DAsync(work, nw * word_bytes, d_in, in_stride * word_bytes, nw * word_bytes, batch, hipMemcpyDeviceToDevice, stream),
                     LW_ERR_LAUNCH);
    for (int q = 0; q < sc.npass; q++) {
        const PassStep &st = sc.step[q];
        const bool from_in = st.src == PASS_IN, to_out = st.dst == PASS_OUT;
        const void *in = from_in ? d_in : work;
        void *out = to_out ? d_out : work;
        if (st.r > NTT_MAX_R || (st.lo && in == out)) {
            if (st.r > NTT_MAX_R) set_error("internal: NTT pass of %u stages", st.r);
            else set_error("internal: last NTT pass would run in place");
            return LW_ERR_BAD_ARG;
        }
        hipEvent_t pe = c.prof_begin(stream);
        const char *name = launch(st, in, out, from_in ? in_stride : nw, to_out ? out_stride : nw, dim3(1u << (Lw - st.r - st.logC), batch));
        c.prof_end(name, pe, stream);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    return LW_OK;
}

}  // namespace lw
