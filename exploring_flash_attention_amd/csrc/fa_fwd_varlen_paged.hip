// fa_fwd_varlen_paged.hip -- launchers of the variable-length forward with a paged key side
// (chunked and prefix-cached prefill against a block-table KV cache, read in place): q / o are
// [T, H, d] described by cu_seqlens; k / v are pools [num_blocks, page_size, H_kv, d] (any strides
// {block, head, row}), key j of sequence b is row j % page_size of block
// clamp(block_table[b][j / page_size], 0, num_blocks - 1), and the sequence has
// clamp(seqused_k[b], 0, max_seqlen_k) keys -- all int32 arrays on the device, nothing read on the
// host.  Causal: bottom-right aligned, as fa_fwd_varlen_kv.hip; a row that sees no key is zeros.
// fa_fwd_kernel (fa_fwd_kernel.hpp) with VARLEN = KVLEN = PAGED = true: the instantiations of
// fa_fwd_varlen_kv.hip otherwise -- final mode, TAIL, STRIDED, GQA = true with kv_group = 1 for MHA,
// bf16 / fp16, d = 32 / 64 / 128 / 256 -- with the same tiles in the same order (bitwise the result
// of fa_fwd_varlen_kv on the cache gathered in table order).  A translation unit of its own, so
// that the instantiations of the other ones compile to what they did before.
//
// Grid: B * H * ceil(max_seqlen / 128) work items, as fa_fwd_varlen.hip: the query side sizes it.
#include "fa_fwd_kernel.hpp"

namespace fa {

template <typename T, int D, bool CAUSAL>
static hipError_t launch_varlen_paged_one(const FwdArgs& a, hipStream_t s) {
    const int64_t nblk = (int64_t)a.nqt * a.BH;
    static const char* const names[2][2] = {
        {"fa_fwd_kernel<final, varlen, paged>", "fa_fwd_kernel<final, varlen, paged, gqa>"},
        {"fa_fwd_kernel<final, varlen, paged, causal>", "fa_fwd_kernel<final, varlen, paged, causal, gqa>"}};
    note_kernel(names[CAUSAL ? 1 : 0][a.kv_group > 1 ? 1 : 0], nblk);
    hipLaunchKernelGGL((fa_fwd_kernel<T, T, D, kFinal, true, true, CAUSAL, true, true, true, true>),
                       dim3((unsigned)nblk), dim3(kThreads), fwd_lds_bytes(D), s, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_varlen_paged_d(int d, bool causal, const FwdArgs& a, hipStream_t s) {
    switch (d) {
        case 32: return causal ? launch_varlen_paged_one<T, 32, true>(a, s) : launch_varlen_paged_one<T, 32, false>(a, s);
        case 64: return causal ? launch_varlen_paged_one<T, 64, true>(a, s) : launch_varlen_paged_one<T, 64, false>(a, s);
        case 128: return causal ? launch_varlen_paged_one<T, 128, true>(a, s) : launch_varlen_paged_one<T, 128, false>(a, s);
        case 256: return causal ? launch_varlen_paged_one<T, 256, true>(a, s) : launch_varlen_paged_one<T, 256, false>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fwd_varlen_paged(Elem t, int d, bool causal, const FwdArgs& a, hipStream_t s) {
    if (!a.strided || a.nsplit != 1 || !a.cu_seqlens || !a.seqused_k || !a.block_table || a.kv_group < 1 || a.H <= 0 ||
        a.H % a.kv_group || a.BH % a.H || a.max_seqlen <= 0 || a.total_rows <= 0 || a.max_seqlen_k <= 0 || a.nqt <= 0 ||
        (int64_t)a.nqt * a.BH >= (int64_t)1 << 31)
        return hipErrorInvalidValue;
    // whole tiles per page (a tile's descriptor never straddles two blocks), a pool to clamp into, a
    // table row that holds the pages of max_seqlen_k keys
    if (a.page_size <= 0 || a.page_size % 64 || a.num_blocks <= 0 || a.block_stride <= 0 ||
        a.table_stride < ((int64_t)a.max_seqlen_k + a.page_size - 1) / a.page_size)
        return hipErrorInvalidValue;
    if (t == Elem::BF16) return launch_varlen_paged_d<__bf16>(d, causal, a, s);
    if (t == Elem::F16) return launch_varlen_paged_d<_Float16>(d, causal, a, s);
    return hipErrorInvalidValue;
}

}  // namespace fa
