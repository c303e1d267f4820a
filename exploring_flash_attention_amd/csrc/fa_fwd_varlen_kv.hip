// fa_fwd_varlen_kv.hip -- launchers of the variable-length forward with key lengths of their own
// (chunked prefill against a prefix, ragged cross-attention): q / o are [Tq, H, d] described by
// cu_seqlens, k / v [Tk, H_kv, d] described by cu_seqlens_k (and, optionally, seqused_k), both
// int32 arrays on the device.  Causal: query position i of a sequence sees keys j <= i + Lk - Lq
// (bottom-right aligned); a row that sees no key is written as zeros.
// fa_fwd_kernel (fa_fwd_kernel.hpp) with VARLEN = KVLEN = true: the instantiations of
// fa_fwd_varlen.hip otherwise -- final mode, TAIL, STRIDED, GQA = true with kv_group = 1 for MHA,
// bf16 / fp16, d = 32 / 64 / 128 / 256.  A translation unit of its own, so that the instantiations
// of the other ones compile to what they did before.
//
// Grid: B * H * ceil(max_seqlen / 128) work items, as fa_fwd_varlen.hip: the query side sizes it.
#include "fa_fwd_kernel.hpp"

namespace fa {

template <typename T, int D, bool CAUSAL>
static hipError_t launch_varlen_kv_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    static const char* const names[2][2] = {
        {"fa_fwd_kernel<final, varlen, kv>", "fa_fwd_kernel<final, varlen, kv, gqa>"},
        {"fa_fwd_kernel<final, varlen, kv, causal>", "fa_fwd_kernel<final, varlen, kv, causal, gqa>"}};
    note_kernel(names[CAUSAL ? 1 : 0][a.kv_group > 1 ? 1 : 0], nblk);
    hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, true, CAUSAL, true, true, true>), dim3((unsigned)nblk),
                       dim3(kThreads), fwd_lds_bytes(D), s, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_varlen_kv_d(int d, bool causal, const FwdArgs& a, hipStream_t s) {
    switch (d) {
        case 32: return causal ? launch_varlen_kv_one<T, 32, true>(a, s) : launch_varlen_kv_one<T, 32, false>(a, s);
        case 64: return causal ? launch_varlen_kv_one<T, 64, true>(a, s) : launch_varlen_kv_one<T, 64, false>(a, s);
        case 128: return causal ? launch_varlen_kv_one<T, 128, true>(a, s) : launch_varlen_kv_one<T, 128, false>(a, s);
        case 256: return causal ? launch_varlen_kv_one<T, 256, true>(a, s) : launch_varlen_kv_one<T, 256, false>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwd_varlen_kv(Elem t, int d, bool causal, const FwdArgs& a, hipStream_t s) {
    if (!a.strided || a.nsplit != 1 || !a.cu_seqlens || !a.cu_seqlens_k || a.kv_group < 1 || a.H <= 0 ||
        a.H % a.kv_group || a.BH % a.H || a.max_seqlen <= 0 || a.total_rows <= 0 || a.max_seqlen_k <= 0 ||
        a.total_rows_k < 0 || a.nqt <= 0 || (int64_t)a.nqt * a.BH >= (int64_t)1 << 31)
        return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_varlen_kv_d<__bf16>(d, causal, a, s);
    if (t == Elem::F16) return launch_varlen_kv_d<_Float16>(d, causal, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
