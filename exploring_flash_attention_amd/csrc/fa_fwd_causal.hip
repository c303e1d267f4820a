// fa_fwd_causal.hip -- launchers of the causal forward: fa_fwd_kernel (fa_fwd_kernel.hpp) with
// CAUSAL = true, final mode, contiguous [B, H, L, d] bf16 / fp16 tensors, Lq = Lk.  A
// translation unit of its own, so that the non-causal instantiations of fa_fwd.hip and
// fa_fwd_strided.hip compile to what they did before the causal mode existed.
//
// Every head dim runs the 32x32x16 kernel here, d = 128 included: the 16x16x32 kernels and the
// chain kernel carry hand-counted waits and a pinned schedule with no place for a mask.  Grid,
// LDS bytes and launch bounds are those of the non-causal kernel of the same d and key tail.
#include "fa_fwd_kernel.hpp"

namespace fa {

template <typename T, int D>
static hipError_t launch_causal_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    const int lds = fwd_lds_bytes(D);
    note_kernel("fa_fwd_kernel<final, causal>", nblk);
    // the key tail (and with it the clamped DMA descriptor) exists only in the last query tile,
    // among the tiles the causal mask covers; the no-tail specialisation as in fa_fwd.hip
    if (a.Lk % bk_for(D) || !(kNoTailMask & d_bit(D)))
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, false, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    else
        hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, false, false, true>), dim3((unsigned)nblk),
                           dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_causal_d(int d, const FwdArgs& a, hipStream_t s) {
    switch (d) {
        case 32: return launch_causal_one<T, 32>(a, s);
        case 64: return launch_causal_one<T, 64>(a, s);
        case 128: return launch_causal_one<T, 128>(a, s);
        case 256: return launch_causal_one<T, 256>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwd_causal(Elem t, int d, const FwdArgs& a, hipStream_t s) {
    if (a.strided || a.nsplit != 1 || a.Lq != a.Lk) return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_causal_d<__bf16>(d, a, s);
    if (t == Elem::F16) return launch_causal_d<_Float16>(d, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
