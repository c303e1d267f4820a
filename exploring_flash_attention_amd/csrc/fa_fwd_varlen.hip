// fa_fwd_varlen.hip -- launchers of the variable-length (token-packed) forward: q / o are
// [T, H, d], k / v [T, H_kv, d] with element strides {token, head}, and an int32 cu_seqlens
// [B + 1] on the device says which token rows belong to which sequence (Lq = Lk per sequence).
// fa_fwd_kernel (fa_fwd_kernel.hpp) with VARLEN = true: final mode, TAIL (lengths are runtime
// values), STRIDED (rows through a runtime stride), causal or not, bf16 / fp16, d = 32 / 64 /
// 128 / 256 -- d = 128 on the 32x32x16 kernel too, as in fa_fwd_causal.hip.  MHA runs the
// GQA = true instantiation with kv_group = 1 (half the kernels; the group only divides the head
// index for the K / V base).  A translation unit of its own, so that the instantiations of the
// other ones compile to what they did before.
//
// Grid: B * H * ceil(max_seqlen / 128) work items; an item whose query tile starts at or past its
// sequence's length returns at once (the host never sees the lengths, so it cannot size the grid
// to them).
#include "fa_fwd_kernel.hpp"

namespace fa {

template <typename T, int D, bool CAUSAL>
static hipError_t launch_varlen_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    static const char* const names[2][2] = {
        {"fa_fwd_kernel<final, varlen>", "fa_fwd_kernel<final, varlen, gqa>"},
        {"fa_fwd_kernel<final, varlen, causal>", "fa_fwd_kernel<final, varlen, causal, gqa>"}};
    note_kernel(names[CAUSAL ? 1 : 0][a.kv_group > 1 ? 1 : 0], nblk);
    hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, true, CAUSAL, true, true>), dim3((unsigned)nblk),
                       dim3(kThreads), fwd_lds_bytes(D), s, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_varlen_d(int d, bool causal, const FwdArgs& a, hipStream_t s) {
    switch (d) {
        case 32: return causal ? launch_varlen_one<T, 32, true>(a, s) : launch_varlen_one<T, 32, false>(a, s);
        case 64: return causal ? launch_varlen_one<T, 64, true>(a, s) : launch_varlen_one<T, 64, false>(a, s);
        case 128: return causal ? launch_varlen_one<T, 128, true>(a, s) : launch_varlen_one<T, 128, false>(a, s);
        case 256: return causal ? launch_varlen_one<T, 256, true>(a, s) : launch_varlen_one<T, 256, false>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwd_varlen(Elem t, int d, bool causal, const FwdArgs& a, hipStream_t s) {
    if (!a.strided || a.nsplit != 1 || !a.cu_seqlens || a.kv_group < 1 || a.H <= 0 || a.H % a.kv_group ||
        a.BH % a.H || a.max_seqlen <= 0 || a.total_rows <= 0 || a.nqt <= 0 ||
        (int64_t)a.nqt * a.BH >= (int64_t)1 << 31)
        return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_varlen_d<__bf16>(d, causal, a, s);
    if (t == Elem::F16) return launch_varlen_d<_Float16>(d, causal, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
