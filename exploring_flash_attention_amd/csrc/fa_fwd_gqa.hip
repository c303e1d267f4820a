// fa_fwd_gqa.hip -- launchers of the grouped-query forward: K and V hold H_kv = H / G heads and
// query head h reads K/V head h / G (FwdArgs::kv_group = G > 1).  Final mode, contiguous
// [B, H, L, d] q / o and [B, H_kv, L, d] k / v, bf16 / fp16, causal or not.  The GQA = true
// instantiations of fa_fwd_kernel, fa_fwd16_kernel and fa_fwd16_chain_kernel differ from the
// others in the K / V base of a work item only.  A translation unit of its own, so that the
// instantiations of fa_fwd.hip, fa_fwd_strided.hip and fa_fwd_causal.hip compile to what they
// did before.
//
// Dispatch is that of an MHA call of the same B*H, L, d: launch_one's rule (fa_fwd.hip) without
// the mask, launch_causal_one's (fa_fwd_causal.hip) with it.
#include "fa_fwd_kernel.hpp"
#include "fa_fwd16_kernel.hpp"
#include "fa_fwd16_chain.hpp"

namespace fa {

template <typename T, int D>
static hipError_t launch_gqa_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    const int lds = fwd_lds_bytes(D);
    if constexpr (D == 128) {
        // the chain kernel and the 16x16x32 kernel under the conditions of fa_fwd.hip's launch_one
        const int64_t grid = 2 * (int64_t)device_cus(s) / 8 * 8;
        if (a.Lk % 128 == 0 && a.Lk >= 256 && a.Lq % kBQ == 0 && nblk >= grid && grid >= 8 &&
            nblk < (int64_t)1 << 31) {
            note_kernel("fa_fwd16_chain_kernel<final, gqa>", grid);
            hipLaunchKernelGGL((fa_fwd16_chain_kernel<T, kFinal, true>), dim3((unsigned)grid), dim3(kThreads),
                               lds, s, a, (int)nblk);
            return hipGetLastError();
        }
        if (a.Lk % bk_for(D) == 0) {
            note_kernel("fa_fwd16_kernel<final, gqa>", nblk);
            hipLaunchKernelGGL((fa_fwd16_kernel<T, T, D, kFinal, false, true>), dim3((unsigned)nblk),
                               dim3(kThreads), lds, s, a);
            return hipGetLastError();
        }
    }
    note_kernel("fa_fwd_kernel<final, gqa>", nblk);
    if (a.Lk % bk_for(D) || !(kNoTailMask & d_bit(D)))
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, false, false, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, false, false, false, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

template <typename T, int D>
static hipError_t launch_gqa_causal_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    const int lds = fwd_lds_bytes(D);
    note_kernel("fa_fwd_kernel<final, causal, gqa>", nblk);
    if (a.Lk % bk_for(D) || !(kNoTailMask & d_bit(D)))
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, false, true, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, false, false, true, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_gqa_d(int d, bool causal, const FwdArgs& a, hipStream_t s) {
    switch (d) {
        case 32: return causal ? launch_gqa_causal_one<T, 32>(a, s) : launch_gqa_one<T, 32>(a, s);
        case 64: return causal ? launch_gqa_causal_one<T, 64>(a, s) : launch_gqa_one<T, 64>(a, s);
        case 128: return causal ? launch_gqa_causal_one<T, 128>(a, s) : launch_gqa_one<T, 128>(a, s);
        case 256: return causal ? launch_gqa_causal_one<T, 256>(a, s) : launch_gqa_one<T, 256>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwd_gqa(Elem t, int d, bool causal, const FwdArgs& a, hipStream_t s) {
    if (a.strided || a.nsplit != 1 || a.Lq != a.Lk || a.kv_group < 2 || a.BH % a.kv_group) return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_gqa_d<__bf16>(d, causal, a, s);
    if (t == Elem::F16) return launch_gqa_d<_Float16>(d, causal, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
